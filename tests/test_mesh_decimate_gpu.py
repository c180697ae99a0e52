"""Mesh decimation on the GPU (mnerf_mesh_decimate, matchnerf_amd/csrc/mesh_finish.hip) against the numpy restatement of
tests/mesh_decimate_helpers.py.

EXACTLY the restatement's: vertex_map, both counts, the faces, the order of the new vertices, and the columns w r g b 0 bit for bit
(sums of doubles in a stated order and one division).  Positions: every component within ONE fp32 ulp of the restatement's - both
sides solve a system of condition <= 1001 in float64, so they agree to about 1e-13 of a cell and can differ only where the two
doubles straddle an fp32 rounding boundary; the number of components that differ at all is printed, not gated (measured: 0 on every
mesh and grid of this file).  Every output lies between guard regions that must stay untouched, and rows beyond the counts keep
their sentinel."""
import numpy as np
import pytest
import torch

import mesh_decimate_helpers as D
import mesh_finish_helpers as H
import mesh_helpers as M
from test_mesh_finish_gpu import SENTINELS, Guarded, _bits, _cuda, _device_two_spheres

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from matchnerf_amd import hip as h
    h.load()
    assert torch.cuda.is_available(), "the gpu-marked tests need a GPU"
    return h


def _decimate(hip, vertices, faces, origin, cell, dims, vertex_rows=None, face_rows=None):
    """host arrays -> guarded outputs of exactly the given rows (default: the input's) -> vertices, faces, vertex_map (numpy, all rows),
    counts"""
    dv, df = _cuda(vertices), _cuda(faces)
    n_vertices, n_faces = len(vertices), len(faces)
    vertex_rows = n_vertices if vertex_rows is None else vertex_rows
    face_rows = n_faces if face_rows is None else face_rows
    adjacency = hip.mesh_adjacency(df, n_vertices)
    v, f, m = Guarded(8 * vertex_rows, torch.float32), Guarded(3 * face_rows, torch.int32), Guarded(n_vertices, torch.int32)
    c = Guarded(2, torch.int64)
    hip.mesh_decimate(dv, df, adjacency, origin, cell, dims, v.t.view(vertex_rows, 8), f.t.view(face_rows, 3), m.t, c.t)
    torch.cuda.synchronize()
    assert v.untouched() and f.untouched() and m.untouched() and c.untouched()
    assert torch.equal(dv.view(torch.int32), _cuda(vertices).view(torch.int32)) and torch.equal(df, _cuda(faces))  # inputs not written
    return v.t.cpu().numpy().reshape(-1, 8), f.t.cpu().numpy().reshape(-1, 3), m.t.cpu().numpy(), [int(x) for x in c.t.cpu()]


def _assert_is_restatement(what, got, want):
    """(vertices, faces, vertex_map, counts) of _decimate with capacities of the input's sizes against D.decimate's dict -> the number
    of position components that differ at all"""
    got_v, got_f, got_map, counts = got
    nv, nf = len(want["vertices"]), len(want["faces"])
    assert counts == [nv, nf], (what, counts, nv, nf)
    assert np.array_equal(got_map, want["vertex_map"]), what
    assert np.array_equal(got_f[:nf], want["faces"]), what
    assert np.array_equal(_bits(got_v[:nv, 3:]), _bits(want["vertices"][:, 3:])), what  # w r g b 0: bit for bit
    assert D.one_ulp_apart(got_v[:nv, :3], want["vertices"][:, :3]).all(), what
    assert (got_v[nv:] == SENTINELS[torch.float32]).all() and (got_f[nf:] == SENTINELS[torch.int32]).all(), what
    return int((_bits(got_v[:nv, :3]) != _bits(want["vertices"][:, :3])).sum())


# ------------------------------------------------------------------------------------------------ the small meshes
@pytest.mark.parametrize("name", list(H.small_meshes()))
def test_small_meshes_are_the_restatement(hip, name):
    vertices, faces = H.small_meshes()[name]
    edge = D.mean_edge(vertices, faces)
    for factor in (1.5, 3.0, 8.0):
        origin, cell, dims = D.grid_of(vertices, factor * edge)
        want = D.decimate(vertices, faces, origin, cell, dims)
        differing = _assert_is_restatement((name, factor), _decimate(hip, vertices, faces, origin, cell, dims), want)
        print(f"decimate {name} at {factor} edges, grid {dims}: {len(vertices)} -> {len(want['vertices'])} vertices, {len(faces)} -> "
              f"{len(want['faces'])} triangles; {differing} of {3 * len(want['vertices'])} position components differ by one ulp")
    origin, cell, dims = D.grid_of(vertices, 4.0 * H.extent_of(vertices))  # one cell
    got = _decimate(hip, vertices, faces, origin, cell, dims)
    assert dims == (1, 1, 1) and got[3] == [1, 0] and not got[2].any()
    _assert_is_restatement((name, "one cell"), got, D.decimate(vertices, faces, origin, cell, dims))


# ------------------------------------------------------------------------------------------------ both scan levels, cells and vertices
def _long_strip(n):
    """a strip of n vertices (seeded permutation of the rows) along x over a grid of n x 1 x 1 unit cells: the x of the k-th vertex
    along the strip is the k-th smallest of n seeded positions in [0, n), so occupied and empty cells alternate irregularly"""
    vertices, faces = H.strip(n, 5)
    vertices = vertices.copy()
    along = np.rint(vertices[:, 0] / 0.5).astype(np.int64)
    assert np.array_equal(np.sort(along), np.arange(n))
    vertices[:, 0] = np.sort(np.random.default_rng(n).random(n) * n)[along]
    return vertices, faces, (0.0, -8.0, -8.0), 1.0, (n, 1, 1)


@pytest.mark.parametrize("n", H.BOUNDARY_SIZES)
def test_strip_across_the_scan_boundaries_of_cells_and_vertices(hip, n):
    vertices, faces, origin, cell, dims = _long_strip(n)
    want = D.decimate(vertices, faces, origin, cell, dims)
    occupied = len(want["vertices"])
    assert 0.5 * n < occupied < 0.75 * n and want["count"].max() >= 3  # about 1 - 1 / e of the cells
    differing = _assert_is_restatement(n, _decimate(hip, vertices, faces, origin, cell, dims), want)
    print(f"decimate strip {n}: {occupied} occupied cells, {len(want['faces'])} of {len(faces)} triangles; {differing} components differ")


# ------------------------------------------------------------------------------------------------ capacities, dropped rows
def test_capacities_cut_rows_not_counts(hip):
    vertices, faces = H.two_spheres()
    origin, cell, dims = D.grid_of(vertices, 3.0 * D.mean_edge(vertices, faces))
    full_v, full_f, full_map, counts = _decimate(hip, vertices, faces, origin, cell, dims)
    half = (counts[0] // 2, counts[1] // 2)
    assert half[0] > 4 and half[1] > 4
    part_v, part_f, part_map, part_counts = _decimate(hip, vertices, faces, origin, cell, dims, *half)  # (guards asserted)
    assert part_counts == counts and np.array_equal(part_map, full_map)
    assert np.array_equal(_bits(part_v), _bits(full_v[:half[0]])) and np.array_equal(part_f, full_f[:half[1]])
    # capacity 0 with NULL outputs, and no vertex_map
    dv, df = _cuda(vertices), _cuda(faces)
    none_v, none_f = torch.empty(0, 8, device="cuda"), torch.empty(0, 3, dtype=torch.int32, device="cuda")
    assert none_v.data_ptr() == 0 and none_f.data_ptr() == 0
    _, _, totals = hip.mesh_decimate(dv, df, hip.mesh_adjacency(df, len(vertices)), origin, cell, dims, none_v, none_f)
    assert [int(x) for x in totals.cpu()] == counts


def test_dropped_rows_and_duplicates_of_both_orientations(hip):
    vertices, faces, origin, cell, dims = D.dropped_case()
    got = _decimate(hip, vertices, faces, origin, cell, dims)
    _assert_is_restatement("dropped", got, D.decimate(vertices, faces, origin, cell, dims))
    assert got[2].tolist() == [0, 1, 2, 0, 1, 2, -1, 3] and got[1][:2].tolist() == [[0, 1, 2], [1, 2, 3]] and got[3] == [4, 2]
    assert np.isfinite(got[0][:4]).all()


def test_vertices_without_triangles_and_the_empty_mesh(hip):
    from matchnerf_amd import fusion
    vertices = H.degenerate()[0]
    none = np.zeros((0, 3), np.int32)
    got = _decimate(hip, vertices, none, (-0.5, -0.5, -0.5), 2.0, (3, 3, 3))
    want = D.decimate(vertices, none, (-0.5, -0.5, -0.5), 2.0, (3, 3, 3))
    assert _assert_is_restatement("no triangles", got, want) == 0 and got[3][1] == 0 and 1 < got[3][0] < 7
    assert not want["lam"].any()  # no area at all: the representatives are the means
    none_v, none_f = torch.empty(0, 8, device="cuda"), torch.empty(0, 3, dtype=torch.int32, device="cuda")
    out = fusion.decimate(none_v, none_f, 1.0)
    assert out[0].shape == (0, 8) and out[1].shape == (0, 3)
    assert fusion.finish(none_v, none_f, smooth=1, decimate_cell=1.0)[0].shape == (0, 8)


# ------------------------------------------------------------------------------------------------ determinism, the module's functions
def _same_bytes(a, b):
    return all(x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def test_two_runs_give_the_same_bytes(hip):
    from matchnerf_amd import fusion
    vertices, faces = _device_two_spheres(hip)
    voxel = H.TWO_SPHERES["voxel"]
    runs = [fusion.decimate(vertices, faces, 2.5 * voxel) for _ in range(2)]
    assert _same_bytes(*runs) and 0 < runs[0][1].shape[0] < faces.shape[0] and 0 < runs[0][0].shape[0] < vertices.shape[0]
    # the grid of the finite bounding box: the restatement on the box fusion.decimate computed
    host_v, host_f = vertices.cpu().numpy(), faces.cpu().numpy()
    lo, hi = host_v[:, :3].min(0).astype(np.float64), host_v[:, :3].max(0).astype(np.float64)
    cell = 2.5 * voxel
    want = D.decimate(host_v, host_f, tuple(lo), cell, tuple(int(np.floor((hi[a] - lo[a]) / cell)) + 1 for a in range(3)))
    assert np.array_equal(runs[0][1].cpu().numpy(), want["faces"]) and D.one_ulp_apart(runs[0][0].cpu().numpy(), want["vertices"]).all()
    small = int(np.unique(H.components(H.two_spheres()[1], vertices.shape[0])[2])[1])
    args = dict(min_component=small + 1, smooth=3, decimate_cell=2.0 * voxel)
    runs = [fusion.finish(vertices, faces, **args) for _ in range(2)]
    assert _same_bytes(*runs)
    # finish is its stages, decimation last
    staged = fusion.decimate(*fusion.finish(vertices, faces, min_component=small + 1, smooth=3), 2.0 * voxel)
    assert _same_bytes(runs[0], staged) and runs[0][1].shape[0] < faces.shape[0] - small
    # decimate_cell = 0: what finish returned before it had the argument
    for kwargs in (dict(), dict(min_component=small + 1, smooth=3), dict(smooth=2)):
        assert _same_bytes(fusion.finish(vertices, faces, decimate_cell=0.0, **kwargs), fusion.finish(vertices, faces, **kwargs))
    assert fusion.finish(vertices, faces, decimate_cell=0.0) == (vertices, faces)


def test_decimated_two_sphere_volume_through_the_module(hip, tmp_path):
    """what fusion.mesh(..., decimate=3) applies to the mesher's output: the grid of the volume, cells of 3 voxels"""
    from matchnerf_amd import fusion
    vertices, faces = _device_two_spheres(hip)
    t = H.TWO_SPHERES
    dims = tuple(int(np.ceil(n / 3)) for n in t["dims"])
    new_v, new_f = fusion.finish(vertices, faces, decimate_cell=3 * t["voxel"], decimate_origin=t["origin"], decimate_dims=dims)
    print(f"two spheres at 3 voxels: {vertices.shape[0]} -> {new_v.shape[0]} vertices, {faces.shape[0]} -> {new_f.shape[0]} triangles")
    assert 0 < new_f.shape[0] < faces.shape[0] and new_v.shape[0] < vertices.shape[0]
    want = D.decimate(vertices.cpu().numpy(), faces.cpu().numpy(), t["origin"], 3 * t["voxel"], dims)
    assert np.array_equal(new_f.cpu().numpy(), want["faces"]) and D.one_ulp_apart(new_v.cpu().numpy(), want["vertices"]).all()
    xyz = new_v[:, :3].cpu().numpy().astype(np.float64)
    box = np.array(t["origin"]) + np.array(t["dims"]) * t["voxel"]
    assert (xyz >= np.array(t["origin"])).all() and (xyz <= box).all()  # every vertex inside the volume's box
    path = tmp_path / "decimated.ply"
    normals = fusion.vertex_normals(new_v, new_f)
    assert fusion.write_ply(str(path), new_v, new_f, normals) == new_v.shape[0]
    got_xyz, got_n, _, got_f = H.read_ply(path)
    assert np.array_equal(got_xyz, new_v[:, :3].cpu().numpy()) and np.array_equal(got_f, new_f.cpu().numpy())
    assert np.array_equal(got_n, normals[:, :3].cpu().numpy())
    centre, radius = t["big"]
    radial = xyz - np.array(centre)
    big = np.linalg.norm(radial, axis=1) < radius + 1.5 * t["voxel"]  # (the small sphere is more than that away)
    n = normals[:, :3].cpu().numpy().astype(np.float64)
    nonzero = np.linalg.norm(n, axis=1) > 0
    assert big.sum() > 20 and (big & nonzero).sum() > 20 and ((n * radial).sum(1)[big & nonzero] > 0).all()


def test_fusion_mesh_decimates_on_the_grid_of_its_volume(hip):
    from matchnerf_amd import fusion
    import fusion_helpers as F
    k, h, w = 5, 24, 32
    s = F.scene(k, h, w, False)
    views, depth, rgb = [hip.make_view(c["extr"], c["intr"], c["near"], c["far"]) for c in s["cams"]], _cuda(s["depth"]), _cuda(M.scene_colours(k, h, w))
    auto = fusion.mesh(views, depth, None, rgb, (h, w), False, resolution=40)
    xyz = auto[0][:, :3].double().cpu().numpy()
    voxel = float((xyz.max(0) - xyz.min(0)).max()) / 36
    bounds = (tuple(xyz.min(0) - 4 * voxel), tuple(xyz.max(0) + 4 * voxel))
    grid = dict(bounds=bounds, voxel=voxel)
    plain = fusion.mesh(views, depth, None, rgb, (h, w), False, **grid)
    assert _same_bytes(plain, fusion.mesh(views, depth, None, rgb, (h, w), False, decimate=0.0, **grid))
    args = dict(min_component_fraction=0.02, smooth=2)
    got = fusion.mesh(views, depth, None, rgb, (h, w), False, decimate=3, **args, **grid)
    assert _same_bytes(got, fusion.mesh(views, depth, None, rgb, (h, w), False, decimate=3, **args, **grid))
    dims = tuple(max(1, int(np.ceil((bounds[1][a] - bounds[0][a]) / voxel - 1e-9))) for a in range(3))
    want = fusion.finish(*plain, **args, decimate_cell=3 * voxel, decimate_origin=tuple(float(x) for x in bounds[0]),
                         decimate_dims=tuple(int(np.ceil(d / 3)) for d in dims))
    print(f"fusion.mesh decimate=3: {plain[1].shape[0]} -> {got[1].shape[0]} triangles, {plain[0].shape[0]} -> {got[0].shape[0]} vertices")
    assert _same_bytes(got, want) and 0 < got[1].shape[0] < plain[1].shape[0] // 3
    assert int(got[1].min()) >= 0 and int(got[1].max()) < got[0].shape[0] and bool(torch.isfinite(got[0]).all())
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            fusion.mesh(views, depth, None, rgb, (h, w), False, decimate=bad, **grid)


def test_export_mesh_and_the_coach_take_the_option(hip, tmp_path, monkeypatch):
    from test_fusion_gpu import LOOSE, _coach, _model
    opt, model, batch, calls = _model("nonlegacy")
    with torch.no_grad():
        plain = model.export_mesh(batch, views="sources", resolution=48, **LOOSE)
        small = model.export_mesh(batch, views="sources", resolution=48, decimate=3, normals=True, **LOOSE)
        with pytest.raises(ValueError):
            model.export_mesh(batch, views="sources", resolution=48, decimate=-1.0, **LOOSE)
    vertices, faces, normals = small[0]
    assert 0 < faces.shape[0] < plain[0][1].shape[0] and normals.shape == (vertices.shape[0], 4) and bool(torch.isfinite(normals).all())
    loose = ["--nerf.export_geometry=sources", "--nerf.fuse_px_tol=64", "--nerf.fuse_rel_tol=0.9", "--nerf.fuse_min_opacity=0.01",
             "--nerf.fuse_min_views=1", "--nerf.export_mesh", "--nerf.mesh_resolution=48", "--nerf.mesh_normals"]
    c = _coach(tmp_path, monkeypatch, *loose)
    before = H.read_ply(c.export_geometry()["dtu"][1])
    c.opts.nerf.mesh_decimate = 3
    path = c.export_geometry()["dtu"][1]
    first = open(path, "rb").read()
    xyz, nrm, rgb, tri = H.read_ply(path)
    print(f"coach mesh_decimate=3: {len(before[3])} -> {len(tri)} triangles, {len(before[0])} -> {len(xyz)} vertices")
    assert 0 < len(tri) < len(before[3]) and len(xyz) < len(before[0]) and nrm is not None and np.isfinite(xyz).all()
    assert tri.min() >= 0 and tri.max() < len(xyz)
    assert open(c.export_geometry()["dtu"][1], "rb").read() == first  # the same bytes on a second run
    for bad in (-2.0, float("nan")):
        c.opts.nerf.mesh_decimate = bad
        with pytest.raises(ValueError, match="mesh_decimate"):
            c.export_geometry()


# ------------------------------------------------------------------------------------------------ refusals
def test_argument_refusals_precede_any_launch(hip):
    D.assert_refusals(hip)
    vertices, faces = (_cuda(x) for x in H.fan())
    n, t = vertices.shape[0], faces.shape[0]
    adj = hip.mesh_adjacency(faces, n)
    guards = [Guarded(8 * n, torch.float32), Guarded(3 * t, torch.int32), Guarded(n, torch.int32), Guarded(2, torch.int64)]
    out_v, out_f, out_m, out_c = guards[0].t.view(n, 8), guards[1].t.view(t, 3), guards[2].t, guards[3].t
    grid = ((-2.0, -2.0, -2.0), 1.0, (4, 4, 4))
    call = lambda *a, **k: hip.mesh_decimate(*a, **{**dict(vertices_out=out_v, triangles_out=out_f, vertex_map=out_m, counts=out_c), **k})
    nan, inf = float("nan"), float("inf")
    wrong = [lambda: call(vertices, faces, adj, grid[0], 0.0, grid[2]), lambda: call(vertices, faces, adj, grid[0], -1.0, grid[2]),
             lambda: call(vertices, faces, adj, grid[0], nan, grid[2]), lambda: call(vertices, faces, adj, grid[0], inf, grid[2]),
             lambda: call(vertices, faces, adj, (nan, 0.0, 0.0), 1.0, grid[2]), lambda: call(vertices, faces, adj, (0.0, 0.0), 1.0, grid[2]),
             lambda: call(vertices, faces, adj, grid[0], 1.0, (0, 4, 4)), lambda: call(vertices, faces, adj, grid[0], 1.0, (2048, 1024, 1024)),
             lambda: call(vertices, faces, (adj[0][:-1], adj[1]), *grid), lambda: call(vertices, faces, (adj[0], adj[1][:-1]), *grid),
             lambda: call(vertices, faces.long(), adj, *grid), lambda: call(vertices.cpu(), faces, adj, *grid),
             lambda: call(vertices, faces, adj, *grid, vertex_map=out_m[:-1]), lambda: call(vertices, faces, adj, *grid, vertex_map=out_m.long()),
             lambda: call(vertices, faces, adj, *grid, counts=torch.zeros(2, dtype=torch.int32, device="cuda")),
             lambda: call(vertices, faces, adj, *grid, vertices_out=out_v.view(-1)[:-1]),
             lambda: call(vertices, faces, adj, *grid, triangles_out=out_f.long()),
             lambda: call(vertices, faces, adj, *grid, workspace=torch.empty(16, dtype=torch.uint8, device="cuda"))]
    for w in wrong:
        with pytest.raises(hip.MnerfError):
            w()
    torch.cuda.synchronize()
    assert all(g.untouched() for g in guards)
    assert all(bool((g.t == g.value).all()) for g in guards)  # and nothing in between was written either
    call(vertices, faces, adj, *grid)  # the same call without a flaw writes
    torch.cuda.synchronize()
    assert int(out_c[0]) > 0 and all(g.untouched() for g in guards)
