"""Mesh export without a GPU: the restatement of tests/mesh_helpers.py checked against what a mesh of a sphere must be (closed,
consistently wound, of the sphere's topology, on the sphere, of its area) and what an open surface must be; the integrator's
restatement on the analytic scene (few borderline voxels on EVERY case the GPU test runs, fp32 against float64); and the host side:
the ABI additions, every argument refusal, the workspace formula, the PLY writer with faces, the options.

Measured here, float32 against float64 restatement (the GPU gates are max(floor, 8 x these)): S per unit of weight up to 1.01e-6,
RGB per unit of weight up to 1.14e-7, over the cases of ``integrate_cases``; vertex rows of the sphere up to 6.2e-8 of the grid's
extent (the values this file prints with -s)."""
import os

import numpy as np
import pytest

import fusion_helpers as F
import mesh_helpers as M
from helpers import REPO, read_header
from matchnerf_amd import fusion, hip, options

NEW_EXPORTS = ("mnerf_tsdf_integrate", "mnerf_tsdf_mesh_workspace_bytes", "mnerf_tsdf_mesh")
SPHERE_GRIDS = [(12, 11, 13), (24, 24, 24)]


# ------------------------------------------------------------------------------------------------ the mesher's restatement
@pytest.mark.parametrize("dims", SPHERE_GRIDS)
def test_sphere_mesh_is_closed_outward_and_on_the_sphere(dims):
    vol, got = M.sphere_volume(dims), M.sphere_mesh(dims)
    area = M.assert_closed_sphere(got["vertices"], got["faces"], vol["voxel"])
    assert 0.9 < area / (4 * np.pi * M.SPHERE_R ** 2) < 1.0  # a chordal surface of a convex body: below, and near
    # the orders the header defines: strictly ascending keys
    vkey = got["vertex_key"][:, 0] * 7 + got["vertex_key"][:, 1]
    fkey = (got["face_key"][:, 0] * 6 + got["face_key"][:, 1]) * 2 + got["face_key"][:, 2]
    assert (np.diff(vkey) > 0).all() and (np.diff(fkey) > 0).all()
    # float32 restatement: the same connectivity (signs of identical fp32 values), rows within rounding
    got32 = M.sphere_mesh(dims, False, np.float32)
    assert np.array_equal(got32["faces"], got["faces"]) and np.array_equal(got32["vertex_key"], got["vertex_key"])
    e32 = M.vertex_distance(got32["vertices"], got["vertices"], vol["voxel"] * max(dims))
    print(f"sphere {dims}: {len(got['vertices'])} vertices, {len(got['faces'])} faces, area {area:.5f}, fp32 rows {e32:.3e}")
    assert e32 < 1e-6


def test_sphere_area_converges():
    exact = 4 * np.pi * M.SPHERE_R ** 2
    err = []
    for n in (12, 24, 48):
        vol, got = M.sphere_volume((n, n, n)), M.sphere_mesh((n, n, n))
        err.append(exact - M.assert_closed_sphere(got["vertices"], got["faces"], vol["voxel"]))
    print("sphere area deficit at 12, 24, 48:", err)
    assert err[0] > 2 * err[1] > 4 * err[2] > 0  # second order in the voxel: better than halved per doubling


def test_tet_table_rule():
    """each case's polygon uses exactly the tet's sign-changing edges; complementary cases are mirror images"""
    for code in range(16):
        tris = M.tet_case(code)
        crossing = {(p, q) for p in range(4) for q in range(p + 1, 4) if (code >> p & 1) != (code >> q & 1)}
        assert {e for t in tris for e in t} == crossing and len(tris) == (0, 1, 2, 1, 0)[bin(code).count("1")]
        mirror = M.tet_case(15 - code)  # the complement: the same polygon, wound the other way
        assert len(mirror) == len(tris) and {e for t in mirror for e in t} == crossing
        if len(tris) == 1:
            assert mirror[0] in ([tris[0][0], tris[0][2], tris[0][1]], [tris[0][2], tris[0][1], tris[0][0]], [tris[0][1], tris[0][0], tris[0][2]])


def test_open_surface_stops_at_the_invalid_cells():
    dims = (12, 11, 13)
    vol, got, closed = M.sphere_volume(dims, True), M.sphere_mesh(dims, True), M.sphere_mesh(dims)
    assert 0 < len(got["faces"]) < len(closed["faces"]) and not got["cell_valid"].all()
    M.assert_open_surface(got["faces"], got["face_key"][:, 0], got["cell_valid"])
    assert len(np.unique(got["faces"])) == len(got["vertices"])  # every vertex is used by a valid cell
    # the part that remains is the closed mesh's: the same triangles, by position
    rows = {tuple(np.round(closed["vertices"][f, :3].reshape(-1), 9)) for f in closed["faces"]}
    assert all(tuple(np.round(got["vertices"][f, :3].reshape(-1), 9)) in rows for f in got["faces"])
    assert vol["weight"].min() == 0


def test_degenerate_grids_have_no_cells():
    for dims in ((1, 5, 4), (5, 1, 4), (5, 4, 1), (1, 1, 1)):
        nx, ny, nz = dims
        sums = np.ones((nz, ny, nx, 4), np.float32)
        sums[..., 0] = np.where(np.arange(nx * ny * nz).reshape(nz, ny, nx) % 2, 1.0, -1.0)
        got = M.mesh(sums, np.full((nz, ny, nx), 3.0, np.float32), (0.0, 0.0, 0.0), 0.1, 2.0)
        assert got["vertices"].shape == (0, 8) and got["faces"].shape == (0, 3)


# ------------------------------------------------------------------------------------------------ the integrator's restatement
@pytest.mark.parametrize("case", M.integrate_cases(), ids=lambda c: "-".join(str(x) for x in c))
def test_integrator_restatement_stays_under_the_borderline_cap(case):
    """a condition of the GPU comparison, on every case it runs: at most 1 % of the voxels borderline, fp32 equal in weight off
    them, and within the cap that the gate puts on the fp32 restatement"""
    k, h, w, legacy, variant, consistent, grid = case
    r = M.integrate_reference(*case)
    n = r["border"].size
    keep = ~r["border"]
    assert r["border"].sum() <= M.BORDERLINE_CAP * n, (case, int(r["border"].sum()), n)
    assert np.array_equal(r["weight"][keep], r["weight32"][keep])
    e_s, e_rgb = M.volume_distance(r["sums32"], r["weight32"], r["sums"], r["weight"], keep)
    print(f"integrate {case}: {int(r['border'].sum())} of {n} voxels borderline, {(r['weight'] > 0).mean():.3f} updated, "
          f"fp32 restatement S {e_s:.3e} RGB {e_rgb:.3e}")
    assert e_s < 1e-5 and e_rgb < 1e-5
    if grid == "default":  # a non-trivial volume: voxels inside the truncation band, in front of it, and untouched ones
        s, wt = r["sums"][..., 0], r["weight"]
        assert (np.abs(s) < wt).mean() > 0.02 and ((s == wt) & (wt > 0)).any() and (wt == 0).any() and (s < 0).any()
    if grid == "half_outside":
        assert (r["weight"] == 0).mean() > 0.5 and (r["weight"] > 0).any()
    if grid == "single":
        assert r["weight"].shape == (1, 1, 1) and r["weight"][0, 0, 0] == k


def test_integrator_restatement_semantics():
    k, h, w = 3, 24, 32
    r = M.integrate_reference(k, h, w, False)
    s = F.scene(k, h, w, False)
    # the zero surface of S / weight is the scene's: lattice points with |d| small lie within trunc of the plane or the box
    p = M.centres(r["origin"], r["voxel"], r["dims"], np.float64)
    d = np.where(r["weight"] >= 2, r["sums"][..., 0] / np.maximum(r["weight"], 1), np.nan)
    lo, hi = np.array([-0.4, -0.3, -0.6]), np.array([0.3, 0.35, 0.0])
    outside_box = np.linalg.norm(np.maximum(np.maximum(lo - p, p - hi), 0), axis=-1)
    to_surface = np.minimum(np.abs(p[..., 2]), np.where(outside_box > 0, outside_box, np.min(np.minimum(p - lo, hi - p), axis=-1)))
    near = np.abs(d) < 0.2
    assert near.sum() > 50 and (to_surface[near] < r["trunc"]).mean() > 0.95
    # two calls accumulate to one: views 0..1 then 2 on the same volume
    args = (h, w, False)
    first = M.integrate(s["cams"][:2], *args, s["depth"][:2], None, r["rgb"][:2], r["origin"], r["voxel"], r["dims"], r["trunc"])
    both = M.integrate(s["cams"][2:], *args, s["depth"][2:], None, r["rgb"][2:], r["origin"], r["voxel"], r["dims"], r["trunc"],
                       volume=first[:2])
    assert np.array_equal(both[1], r["weight"]) and np.allclose(both[0], r["sums"], rtol=0, atol=1e-12)
    # the mesh of that volume is an open surface of the scene
    got = M.mesh(r["sums"].astype(np.float32), r["weight"].astype(np.float32), r["origin"], r["voxel"], 2.0)
    assert len(got["faces"]) > 100 and len(np.unique(got["faces"])) == len(got["vertices"])
    und, forward, backward = M.edge_uses(got["faces"])
    assert (forward <= 1).all() and (backward <= 1).all()


# ------------------------------------------------------------------------------------------------ host side
def test_exports_and_abi_stay_put():
    header = read_header()
    names = [name for _, name, _ in header.prototypes]
    for name in NEW_EXPORTS:
        assert name in hip.SIGNATURES and name in hip.EXPORTS and name in names, name
    lib = hip.load()
    assert lib.mnerf_abi_version() == 12 == hip.MNERF_ABI_VERSION == header.constants["MNERF_ABI_VERSION"]
    assert len(hip.STRUCTS) == 11 and lib.mnerf_struct_size(11) == -1  # no new struct


def test_argument_refusals_precede_any_hip_call():
    M.assert_refusals(hip)


def test_ply_with_faces_round_trips_and_without_is_unchanged(tmp_path):
    rng = np.random.default_rng(11)
    pts = rng.normal(size=(29, 8)).astype(np.float32)
    pts[:, 4:7] = rng.uniform(0, 1, (29, 3))
    faces = rng.integers(0, 29, (41, 3)).astype(np.int32)
    path = str(tmp_path / "mesh.ply")
    assert fusion.write_ply(path, pts, faces) == 29
    xyz, rgb, got = M.read_ply(path)
    assert np.array_equal(xyz, pts[:, :3]) and np.array_equal(got, faces) and got.dtype == np.int32
    assert np.array_equal(rgb, np.rint(pts[:, 4:7] * 255).astype(np.uint8))
    import torch
    assert fusion.write_ply(path, torch.from_numpy(pts), torch.from_numpy(faces)) == 29 and np.array_equal(M.read_ply(path)[2], faces)
    assert fusion.write_ply(path, pts, np.zeros((0, 3), np.int32)) == 29 and M.read_ply(path)[2].shape == (0, 3)
    with pytest.raises(ValueError):
        fusion.write_ply(path, pts, np.array([[0, 1, 29]]))
    # without faces: the point cloud's file, byte for byte what the writer's format has always been
    cloud = str(tmp_path / "cloud.ply")
    assert fusion.write_ply(cloud, pts) == 29
    blob = open(cloud, "rb").read()
    header = b"ply\nformat binary_little_endian 1.0\nelement vertex 29\nproperty float x\nproperty float y\nproperty float z\n" \
             b"property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n"
    body = b"".join(pts[i, :3].tobytes() + np.rint(pts[i, 4:7] * 255).astype(np.uint8).tobytes() for i in range(29))
    assert blob == header + body
    assert M.read_ply(cloud)[2] is None and np.array_equal(F.read_ply(cloud)[0], pts[:, :3])


def test_options_parse_and_default_to_absent():
    opt = options.load_options("configs/test.yaml", verbose=False)
    names = ("export_mesh", "mesh_resolution", "mesh_voxel", "mesh_trunc", "mesh_min_weight")
    for name in names:
        assert getattr(opt.nerf, name, None) is None and name not in opt.nerf, name
    cmd = options.parse_arguments(["--nerf.export_geometry=sources", "--nerf.export_mesh", "--nerf.mesh_resolution=96",
                                   "--nerf.mesh_voxel=0.02", "--nerf.mesh_trunc=0.1", "--nerf.mesh_min_weight=3"])
    opt = options.override_options(opt, cmd)
    assert opt.nerf.export_geometry == "sources" and opt.nerf.export_mesh is True
    assert (opt.nerf.mesh_resolution, opt.nerf.mesh_voxel, opt.nerf.mesh_trunc, opt.nerf.mesh_min_weight) == (96, 0.02, 0.1, 3)
    with open(os.path.join(REPO, "test.py")) as f:  # the script's docstring names them
        text = f.read()
    assert all("--nerf." + name in text for name in names)


def test_mesh_refuses_before_any_launch():
    with pytest.raises(ValueError, match="at least 2"):
        fusion.mesh([object()], None, None, None, (4, 4), True)
