"""Mesh export on the GPU (matchnerf_amd/csrc/mesh.hip): the TSDF integrator against the float64 restatement of
tests/mesh_helpers.py on the analytic scene, the mesher against the restatement on the SAME fp32 volume and against what a mesh of a
sphere must be, capacities, determinism, argument refusals, and the host paths (fusion.mesh, MatchNeRF.export_mesh,
Coach.export_geometry with nerf.export_mesh).

Gates.  weight: equal on every voxel the restatement does not mark borderline (at most 1 % of a case's voxels, asserted in
tests/test_mesh_cpu.py for every case).  S and RGB where the weights agree: the difference per unit of weight below the larger of 1e-5
and 8 x the difference of the same restatement run in fp32 (itself below 1e-5; measured 5e-7 .. 1.1e-6 for S, 3e-8 .. 1.2e-7 for RGB).
Mesh: counts, the face array and so the vertex order exactly equal (sign tests on identical fp32 values are exact); vertex rows
within the larger of 1e-6 of the grid's extent and 8 x the fp32 restatement's distance (measured 6e-8)."""
import numpy as np
import pytest
import torch

import fusion_helpers as F
import mesh_helpers as M

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = -777.25


@pytest.fixture(scope="module")
def hip():
    from matchnerf_amd import hip as h
    h.load()
    assert torch.cuda.is_available(), "the gpu-marked tests need a GPU"
    return h


def _views(hip, cams):
    return [hip.make_view(c["extr"], c["intr"], c["near"], c["far"]) for c in cams]


def _guarded(n, dtype=torch.float32, value=SENTINEL):
    buf = torch.full((n + 2 * GUARD,), value, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def _guards_untouched(buf, n, value=SENTINEL):
    return bool((buf[:GUARD] == value).all()) and bool((buf[GUARD + n:] == value).all())


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _integrate(hip, r, legacy):
    """the kernel on the inputs of a reference case, 16 views per call, into guarded zeroed buffers -> sums, weight (numpy)"""
    nx, ny, nz = r["dims"]
    n, k = nx * ny * nz, len(r["cams"])
    sbuf, sums = _guarded(4 * n)
    wbuf, weight = _guarded(n)
    sums.zero_(), weight.zero_()
    views, depth, opacity, rgb, counts = _views(hip, r["cams"]), _cuda(r["depth"]), _cuda(r["opacity"]), _cuda(r["rgb"]), _cuda(r["counts"])
    for first in range(0, k, hip.MNERF_MAX_VIEWS):
        g = slice(first, min(first + hip.MNERF_MAX_VIEWS, k))
        hip.tsdf_integrate(views[g], depth[g], rgb[g], r["origin"], r["voxel"], r["dims"], r["trunc"], sums, weight,
                           opacity=None if opacity is None else opacity[g], n_consistent=None if counts is None else counts[g],
                           min_consistent=r["min_consistent"], legacy=legacy, min_opacity=M.MIN_OPACITY)
    torch.cuda.synchronize()
    assert _guards_untouched(sbuf, 4 * n) and _guards_untouched(wbuf, n)
    return sums.cpu().numpy().reshape(nz, ny, nx, 4), weight.cpu().numpy().reshape(nz, ny, nx)


def _mesh(hip, sums, weight, origin, voxel, min_weight, vertex_rows=None, face_rows=None):
    """the kernel on a numpy volume with guarded buffers of exactly the given (default: the needed) rows -> vertices, faces, counts"""
    nz, ny, nx = weight.shape
    dims = (nx, ny, nz)
    s, w = _cuda(sums.astype(np.float32)), _cuda(weight.astype(np.float32))
    if vertex_rows is None:  # a first run for the counts alone: no row is written
        _, _, counts = hip.tsdf_mesh(s, w, origin, voxel, dims, min_weight, torch.empty(0, 8, device="cuda"),
                                     torch.empty(0, 3, dtype=torch.int32, device="cuda"))
        vertex_rows, face_rows = (int(c) for c in counts.cpu())
    vbuf, vertices = _guarded(8 * vertex_rows)
    fbuf, faces = _guarded(3 * face_rows, torch.int32, -777)
    _, _, counts = hip.tsdf_mesh(s, w, origin, voxel, dims, min_weight, vertices.view(-1, 8), faces.view(-1, 3))
    torch.cuda.synchronize()
    assert _guards_untouched(vbuf, 8 * vertex_rows) and _guards_untouched(fbuf, 3 * face_rows, -777)
    return vertices.cpu().numpy().reshape(-1, 8), faces.cpu().numpy().reshape(-1, 3), [int(c) for c in counts.cpu()]


def _assert_mesh_is_the_restatement(hip, sums, weight, origin, voxel, min_weight, what):
    """-> (the kernel's vertices, faces, the float64 restatement)"""
    want, want32 = (M.mesh(sums, weight, origin, voxel, min_weight, dtype) for dtype in (np.float64, np.float32))
    vertices, faces, counts = _mesh(hip, sums, weight, origin, voxel, min_weight)
    assert counts == [len(want["vertices"]), len(want["faces"])], (what, counts)
    assert np.array_equal(want32["faces"], want["faces"])
    assert np.array_equal(faces, want["faces"]), (what, np.argwhere(faces != want["faces"])[:5])
    extent = voxel * max(weight.shape)
    e32 = M.vertex_distance(want32["vertices"], want["vertices"], extent)
    err = M.vertex_distance(vertices, want["vertices"], extent)  # row by row: the vertex ORDER is the restatement's
    print(f"mesh {what}: {counts[0]} vertices, {counts[1]} faces, rows {err:.3e} (fp32 restatement {e32:.3e})")
    assert e32 < 1e-6 and err < max(1e-6, 8 * e32), (what, err, e32)
    assert len(vertices) == 0 or (vertices[:, 7] == 0).all()
    again = _mesh(hip, sums, weight, origin, voxel, min_weight)  # two runs: the same bytes
    assert np.array_equal(again[0].view(np.uint32), vertices.view(np.uint32)) and np.array_equal(again[1], faces)
    return vertices, faces, want


# ------------------------------------------------------------------------------------------------ a. integration
@pytest.mark.parametrize("case", M.integrate_cases(), ids=lambda c: "-".join(str(x) for x in c))
def test_integrate_against_float64(hip, case):
    k, h, w, legacy, variant, consistent, grid = case
    r = M.integrate_reference(*case)
    sums, weight = _integrate(hip, r, legacy)
    keep = ~r["border"]
    assert np.array_equal(weight[keep], r["weight"][keep]), (case, np.argwhere((weight != r["weight"]) & keep)[:5])
    untouched = keep & (r["weight"] == 0)
    assert (sums[untouched] == 0).all()
    e_s, e_rgb = M.volume_distance(sums, weight, r["sums"], r["weight"], keep)
    e32_s, e32_rgb = M.volume_distance(r["sums32"], r["weight32"], r["sums"], r["weight"], keep)
    print(f"integrate {case}: S {e_s:.3e} (fp32 restatement {e32_s:.3e}), RGB {e_rgb:.3e} ({e32_rgb:.3e}), "
          f"{int(r['border'].sum())} of {weight.size} voxels borderline")
    assert r["border"].sum() <= M.BORDERLINE_CAP * weight.size
    assert e32_s < 1e-5 and e_s < max(1e-5, 8 * e32_s), (case, e_s, e32_s)
    assert e32_rgb < 1e-5 and e_rgb < max(1e-5, 8 * e32_rgb), (case, e_rgb, e32_rgb)
    again = _integrate(hip, r, legacy)  # two runs: the same bits
    assert np.array_equal(again[0].view(np.uint32), sums.view(np.uint32)) and np.array_equal(again[1], weight)


def test_integrate_wrapper_refusals(hip):
    r = M.integrate_reference(3, 24, 32, False)
    views, depth, rgb = _views(hip, r["cams"]), _cuda(r["depth"]), _cuda(r["rgb"])
    nx, ny, nz = r["dims"]
    sums, weight = torch.zeros(nz, ny, nx, 4, device="cuda"), torch.zeros(nz, ny, nx, device="cuda")
    args = (r["origin"], r["voxel"], r["dims"], r["trunc"])
    for bad in (dict(depth=depth[:2]), dict(rgb=rgb[:2]), dict(sums=sums[:-1]), dict(weight=weight.double()), dict(opacity=depth[:1]),
                dict(n_consistent=torch.zeros(3, 24, 32, device="cuda")), dict(depth=depth.cpu())):
        kw = dict(dict(depth=depth, rgb=rgb, sums=sums, weight=weight), **bad)
        with pytest.raises(hip.MnerfError):
            hip.tsdf_integrate(views, kw.pop("depth"), kw.pop("rgb"), *args, kw.pop("sums"), kw.pop("weight"), **kw)
    with pytest.raises(hip.MnerfError, match="trunc"):
        hip.tsdf_integrate(views, depth, rgb, r["origin"], r["voxel"], r["dims"], 0.0, sums, weight)
    torch.cuda.synchronize()
    assert not sums.any() and not weight.any()  # nothing was launched


# ------------------------------------------------------------------------------------------------ b. mesher
# 12 x 11 x 13: ragged, 256 does not divide the 1716 points.  64^3 and 65 x 64 x 64: 262 144 and 266 240 points, just under and over
# what ONE workgroup of the scan covers (1024 workgroup counts of 256 points).
@pytest.mark.parametrize("dims", [(12, 11, 13), (64, 64, 64), (65, 64, 64)], ids=str)
def test_mesh_of_the_sphere_is_the_restatement_and_a_sphere(hip, dims):
    vol = M.sphere_volume(dims)
    vertices, faces, want = _assert_mesh_is_the_restatement(hip, vol["sums"], vol["weight"], vol["origin"], vol["voxel"], 2.0, dims)
    area = M.assert_closed_sphere(vertices, faces, vol["voxel"])  # on the GPU's own output
    assert 0.9 < area / (4 * np.pi * M.SPHERE_R ** 2) < 1.0
    colour = 0.5 + 0.5 * np.sin(3.0 * vertices[:, :3].astype(np.float64))  # the colour travels with the position
    assert np.abs(vertices[:, 4:7] - colour).max() < 1.5 * (3.0 * vol["voxel"]) ** 2 / 8 + 1e-5 and (vertices[:, 3] == 3).all()


def test_mesh_with_an_invalid_octant_is_open_there(hip):
    dims = (12, 11, 13)
    vol = M.sphere_volume(dims, True)
    vertices, faces, want = _assert_mesh_is_the_restatement(hip, vol["sums"], vol["weight"], vol["origin"], vol["voxel"], 2.0, "open")
    M.assert_open_surface(faces, want["face_key"][:, 0], want["cell_valid"])  # (the faces are the restatement's, so are their cells)
    assert len(np.unique(faces)) == len(vertices) and np.isfinite(vertices).all()
    # no vertex lies strictly inside the block of zero-weight points
    origin, voxel = np.array(vol["origin"]), vol["voxel"]
    p = M.centres(vol["origin"], voxel, dims, np.float64)[vol["weight"] == 0]
    assert not ((vertices[:, None, :3] > p.min(0) + 1e-6) & (vertices[:, None, :3] < p.max(0) - 1e-6)).all(-1).any()


@pytest.mark.parametrize("dims", [(1, 9, 8), (9, 1, 8), (9, 8, 1), (1, 1, 1)], ids=str)
def test_mesh_of_a_grid_without_cells_is_empty(hip, dims):
    nx, ny, nz = dims
    sums = np.ones((nz, ny, nx, 4), np.float32)
    sums[..., 0] = np.where(np.arange(nx * ny * nz).reshape(nz, ny, nx) % 2, 1.0, -1.0)  # sign changes everywhere
    vertices, faces, counts = _mesh(hip, sums, np.full((nz, ny, nx), 3.0, np.float32), (0.0, 0.0, 0.0), 0.1, 2.0, 4, 4)
    assert counts == [0, 0] and (vertices == SENTINEL).all() and (faces == -777).all()


def test_mesh_of_the_volume_the_integrator_produced(hip):
    case = (3, 24, 32, False, "plain", False, "default")
    r = M.integrate_reference(*case)
    sums, weight = _integrate(hip, r, False)
    vertices, faces, want = _assert_mesh_is_the_restatement(hip, sums, weight, r["origin"], r["voxel"], 2.0, "integrated")
    assert len(faces) > 100 and len(np.unique(faces)) == len(vertices)
    und, forward, backward = M.edge_uses(faces)
    assert (forward <= 1).all() and (backward <= 1).all()
    # the surface is the scene's: the plane z = 0 or the box on it, within the truncation band
    lo, hi = np.array([-0.4, -0.3, -0.6]), np.array([0.3, 0.35, 0.0])
    p = vertices[:, :3].astype(np.float64)
    to_box = np.where(((p >= lo) & (p <= hi)).all(1), np.minimum(p - lo, hi - p).min(1), np.linalg.norm(np.maximum(np.maximum(lo - p, p - hi), 0), axis=1))
    assert (np.minimum(np.abs(p[:, 2]), to_box) < r["trunc"]).mean() > 0.95
    assert vertices[:, 4:7].min() >= 0 and vertices[:, 4:7].max() <= 1 and vertices[:, 3].min() >= 2


def test_mesh_capacities_cut_the_rows_not_the_counts(hip):
    dims = (12, 11, 13)
    vol = M.sphere_volume(dims)
    full_v, full_f, counts = _mesh(hip, vol["sums"], vol["weight"], vol["origin"], vol["voxel"], 2.0)
    half = (counts[0] // 2, counts[1] // 2)
    part_v, part_f, part_counts = _mesh(hip, vol["sums"], vol["weight"], vol["origin"], vol["voxel"], 2.0, *half)  # (guards asserted)
    assert part_counts == counts and half[0] > 0 and half[1] > 0
    assert np.array_equal(part_v.view(np.uint32), full_v[:half[0]].view(np.uint32)) and np.array_equal(part_f, full_f[:half[1]])
    over = _mesh(hip, vol["sums"], vol["weight"], vol["origin"], vol["voxel"], 2.0, counts[0] + 7, counts[1] + 5)
    assert over[2] == counts and np.array_equal(over[1][:counts[1]], full_f) and (over[1][counts[1]:] == -777).all()
    assert (over[0][counts[0]:] == SENTINEL).all()


def test_argument_refusals_precede_any_launch(hip):
    M.assert_refusals(hip)
    vol = M.sphere_volume((12, 11, 13))
    s, w = _cuda(vol["sums"]), _cuda(vol["weight"])
    good = dict(vertices=torch.empty(8, 8, device="cuda"), triangles=torch.empty(8, 3, dtype=torch.int32, device="cuda"))
    for bad in (dict(vertices=torch.empty(9, 7, device="cuda")), dict(triangles=torch.empty(8, 3, dtype=torch.int64, device="cuda")),
                dict(counts=torch.zeros(2, dtype=torch.int32, device="cuda")), dict(workspace=torch.empty(16, dtype=torch.uint8, device="cuda")),
                dict(vertices=torch.empty(8, 8))):
        with pytest.raises(hip.MnerfError):
            hip.tsdf_mesh(s, w, vol["origin"], vol["voxel"], (12, 11, 13), 2.0, **dict(good, **bad))
    with pytest.raises(hip.MnerfError):
        hip.tsdf_mesh(s, w, vol["origin"], vol["voxel"], (12, 11, 12), 2.0, **good)
    with pytest.raises(hip.MnerfError, match="min_weight"):
        hip.tsdf_mesh(s, w, vol["origin"], vol["voxel"], (12, 11, 13), 0.0, **good)


# ------------------------------------------------------------------------------------------------ c. fusion.mesh
def test_fusion_mesh_of_the_analytic_scene(hip, monkeypatch):
    from matchnerf_amd import fusion
    k, h, w = 5, 24, 32
    s = F.scene(k, h, w, False)
    views, depth, rgb = _views(hip, s["cams"]), _cuda(s["depth"]), _cuda(M.scene_colours(k, h, w))
    vertices, faces = fusion.mesh(views, depth, None, rgb, (h, w), False, resolution=40)
    assert vertices.shape[1] == 8 and faces.dtype == torch.int32 and faces.shape[1] == 3 and faces.shape[0] > 500
    assert int(faces.min()) >= 0 and int(faces.max()) < vertices.shape[0] and len(torch.unique(faces)) == vertices.shape[0]
    p = vertices[:, :3].double().cpu().numpy()
    lo, hi = np.array([-0.4, -0.3, -0.6]), np.array([0.3, 0.35, 0.0])
    to_box = np.where(((p >= lo) & (p <= hi)).all(1), np.minimum(p - lo, hi - p).min(1), np.linalg.norm(np.maximum(np.maximum(lo - p, p - hi), 0), axis=1))
    side = float((p.max(0) - p.min(0)).max())
    assert (np.minimum(np.abs(p[:, 2]), to_box) < 4 * side / 40).mean() > 0.9  # within the default truncation of the surface
    again = fusion.mesh(views, depth, None, rgb, (h, w), False, resolution=40)
    assert torch.equal(again[0].view(torch.int32), vertices.view(torch.int32)) and torch.equal(again[1], faces)
    # a first guess that is too small: one more run of the mesher, the same mesh
    monkeypatch.setattr(fusion, "MESH_GUESS_ROWS", 0)
    assert vertices.shape[0] > 1024
    small = fusion.mesh(views, depth, None, rgb, (h, w), False, resolution=40)
    assert torch.equal(small[0].view(torch.int32), vertices.view(torch.int32)) and torch.equal(small[1], faces)
    monkeypatch.undo()
    # explicit bounds and sizes, no consistency pass, 20 views in two groups
    k = 20
    s = F.scene(k, h, w, True)
    views, depth, rgb = _views(hip, s["cams"]), _cuda(s["depth"]), _cuda(M.scene_colours(k, h, w))
    v2, f2 = fusion.mesh(views, depth, torch.ones_like(depth), rgb, (h, w), True, bounds=((-0.9, -0.8, -0.9), (0.9, 0.8, 0.3)), voxel=0.05,
                         trunc=0.15, min_weight=3, consistency=False)
    assert f2.shape[0] > 500 and int(f2.max()) < v2.shape[0] and float(v2[:, 3].min()) >= 3
    box = v2[:, :3].cpu().numpy()
    assert (box.min(0) >= np.array([-0.9, -0.8, -0.9])).all() and (box.max(0) <= np.array([0.9, 0.8, 0.3]) + 0.05).all()
    with pytest.raises(ValueError, match="no box"):
        fusion.mesh(views[:3], depth[:3], None, rgb[:3], (h, w), True, bounds=((1.0, 0.0, 0.0), (0.0, 1.0, 1.0)))


# ------------------------------------------------------------------------------------------------ d. the module and the coach
def test_export_mesh_on_the_synthetic_model(hip):
    from test_fusion_gpu import LOOSE, _model
    opt, model, batch, calls = _model("nonlegacy")
    with pytest.raises(NotImplementedError):  # gradients
        model.export_mesh(batch)
    with torch.no_grad():
        with pytest.raises(TypeError):
            model.export_mesh(batch, tolerance=1.0)
        assert calls == []  # refused before the encoder ran
        meshes = model.export_mesh(batch, views="sources", resolution=48, **LOOSE)
        assert len(calls) == 1  # one encoder pass for the K renders
        again = model.export_mesh(batch, views="sources", resolution=48, **LOOSE)
    assert len(meshes) == 1
    vertices, faces = meshes[0]
    assert vertices.shape[1] == 8 and faces.shape[1] == 3 and faces.dtype == torch.int32
    print(f"export_mesh on the synthetic model: {vertices.shape[0]} vertices, {faces.shape[0]} faces")
    assert faces.numel() == 0 or (int(faces.min()) >= 0 and int(faces.max()) < vertices.shape[0])
    assert torch.equal(again[0][0].view(torch.int32), vertices.view(torch.int32)) and torch.equal(again[0][1], faces)
    with torch.no_grad():
        opt.nerf.depth.param = "inverse"
        with pytest.raises(ValueError, match="inverse"):
            model.export_mesh(batch)


def test_coach_export_geometry_writes_the_mesh_next_to_the_cloud(tmp_path, monkeypatch):
    from test_fusion_gpu import _coach
    loose = ["--nerf.export_geometry=sources", "--nerf.fuse_px_tol=64", "--nerf.fuse_rel_tol=0.9", "--nerf.fuse_min_opacity=0.01",
             "--nerf.fuse_min_views=1"]
    c = _coach(tmp_path, monkeypatch, *loose, "--nerf.export_mesh", "--nerf.mesh_resolution=48")
    written = c.export_geometry()
    assert list(written) == ["dtu"] and len(written["dtu"]) == 2 and written["dtu"][1] == written["dtu"][0][:-4] + "_mesh.ply"
    xyz, rgb, faces = M.read_ply(written["dtu"][1])  # (the reader asserts the header's counts against the body)
    assert np.isfinite(xyz).all() and faces is not None and (len(faces) == 0 or (faces.min() >= 0 and faces.max() < len(xyz)))
    cloud = F.read_ply(written["dtu"][0])
    before = [open(p, "rb").read() for p in written["dtu"]]
    assert c.export_geometry() == written and [open(p, "rb").read() for p in written["dtu"]] == before  # a second run: the same bytes
    # without the option: the files of today, the cloud the same bytes
    out_dir = tmp_path / "outputs" / "geometry" / "geometry" / "dtu"
    for p in out_dir.glob("*.ply"):
        p.unlink()
    c.opts.nerf.export_mesh = False
    assert c.export_geometry() == {"dtu": written["dtu"][:1]} and [p.name for p in out_dir.glob("*.ply")] == [written["dtu"][0].split("/")[-1]]
    assert open(written["dtu"][0], "rb").read() == before[0] and len(cloud[0]) > 0
