"""The brick-sparse TSDF volume on the GPU (matchnerf_amd/csrc/tsdf_sparse.hip).

Gates.  Mark: sandwiched by the float64 restatement of tests/tsdf_sparse_helpers.py - every brick the NEAR voxels that are not
UNSURE ask for is marked, no brick is marked that NEAR-or-UNSURE voxels do not ask for (UNSURE: ``M.integrate``'s borderline voxels and
an sdf within 1e-5 trunc of +trunc).  Table: exactly the ascending enumeration of the device's own marks.  Integrate: every allocated
voxel bitwise the dense kernel's on the same inputs - device against device, no tolerance.  Mesh: counts, vertex rows and faces
bitwise the dense GPU mesher's after the renumbering the header states.  End to end: ``fusion.mesh(sparse=True)`` is ``fusion.mesh()``
with vertices and triangles reordered, bit for bit."""
import numpy as np
import pytest
import torch

import fusion_helpers as F
import mesh_helpers as M
import tsdf_sparse_helpers as S

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


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _groups(hip, r, legacy):
    """the device inputs of a reference case, 16 views per call -> [(views, depth, rgb, kwargs)]"""
    views, depth, opacity, rgb, counts = _views(hip, r["cams"]), _cuda(r["depth"]), _cuda(r["opacity"]), _cuda(r["rgb"]), _cuda(r["counts"])
    out = []
    for first in range(0, len(views), hip.MNERF_MAX_VIEWS):
        g = slice(first, min(first + hip.MNERF_MAX_VIEWS, len(views)))
        out.append((views[g], depth[g], rgb[g], dict(opacity=None if opacity is None else opacity[g],
                                                      n_consistent=None if counts is None else counts[g],
                                                      min_consistent=r["min_consistent"], legacy=legacy, min_opacity=M.MIN_OPACITY)))
    return out


def _mark_and_table(hip, r, legacy):
    """the two kernels on guarded buffers -> marks [bz, by, bx] uint8, table [bz, by, bx], bricks [n], n (numpy) and the device
    tensors (table, bricks)"""
    bx, by, bz = bdims = hip.brick_dims(r["dims"])
    n = bx * by * bz
    mbuf, marks = _guarded(n, torch.uint8, 77)
    marks.zero_()
    for views, depth, _, kw in _groups(hip, r, legacy):
        hip.tsdf_bricks_mark(views, depth, r["origin"], r["voxel"], r["dims"], r["trunc"], marks, **kw)
    tbuf, table = _guarded(n, torch.int32, -777)
    bbuf, bricks = _guarded(n, torch.int32, -777)
    cbuf, count = _guarded(1, torch.int64, -777)
    need = hip.tsdf_bricks_table_workspace_bytes(bdims)
    wbuf, ws = _guarded(need, torch.uint8, 77)
    hip.tsdf_bricks_table(marks, bdims, table, bricks, count, workspace=ws)
    torch.cuda.synchronize()
    assert _guards_untouched(mbuf, n, 77) and _guards_untouched(tbuf, n, -777) and _guards_untouched(bbuf, n, -777)
    assert _guards_untouched(cbuf, 1, -777) and _guards_untouched(wbuf, need, 77)
    n_bricks = int(count.cpu())
    return marks.cpu().numpy().reshape(bz, by, bx), table.cpu().numpy().reshape(bz, by, bx), bricks.cpu().numpy(), n_bricks, (table, bricks)


# ------------------------------------------------------------------------------------------------ a. mark, table, integrate
@pytest.mark.parametrize("case", S.MARK_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_mark_table_and_integrate(hip, case):
    k, h, w, legacy = case[:4]
    r = S.reference(*case)
    marks, table, bricks, n_bricks, (dev_table, dev_bricks) = _mark_and_table(hip, r, legacy)
    # the sandwich
    must, may = S.wanted_bricks(r["near"] & ~r["unsure"]), S.wanted_bricks(r["near"] | r["unsure"])
    assert set(np.unique(marks)) <= {0, 1}
    marked = marks != 0
    print(f"mark {case}: {int(marked.sum())} of {marked.size} bricks marked, {int(must.sum())} required, {int(may.sum())} allowed, "
          f"{int(r['unsure'].sum())} of {r['unsure'].size} voxels unsure")
    assert not (must & ~marked).any(), np.argwhere(must & ~marked)[:5]
    assert not (marked & ~may).any(), np.argwhere(marked & ~may)[:5]
    assert 0 < marked.sum() < marked.size or case[6] == "default"
    # the table: the ascending enumeration of the device's own marks
    want_table, want_bricks = S.table_of(marked)
    assert n_bricks == len(want_bricks) and np.array_equal(table, want_table) and np.array_equal(bricks[:n_bricks], want_bricks)
    assert (bricks[n_bricks:] == -777).all()  # the list's tail is not written
    # integrate: bitwise the dense kernel's voxels
    nx, ny, nz = r["dims"]
    dense_s, dense_w = torch.zeros(nz, ny, nx, 4, device="cuda"), torch.zeros(nz, ny, nx, device="cuda")
    sbuf, sums = _guarded(4 * 512 * n_bricks)
    wbuf, weight = _guarded(512 * n_bricks)
    sums.zero_(), weight.zero_()
    for views, depth, rgb, kw in _groups(hip, r, legacy):
        hip.tsdf_integrate(views, depth, rgb, r["origin"], r["voxel"], r["dims"], r["trunc"], dense_s, dense_w, **kw)
        hip.tsdf_integrate_sparse(views, depth, rgb, r["origin"], r["voxel"], r["dims"], r["trunc"], dev_bricks, n_bricks, sums, weight, **kw)
    torch.cuda.synchronize()
    assert _guards_untouched(sbuf, 4 * 512 * n_bricks) and _guards_untouched(wbuf, 512 * n_bricks)
    want_s, want_w = S.brick_volume(dense_s.cpu().numpy(), dense_w.cpu().numpy(), want_table, poison=False)
    assert np.array_equal(_bits(sums.cpu().numpy()).reshape(want_s.shape), _bits(want_s))
    assert np.array_equal(_bits(weight.cpu().numpy()).reshape(want_w.shape), _bits(want_w))  # (and 0 outside the grid)
    assert want_w.max() >= min(k, 2)
    # every voxel the dense volume updates with t < 1 somewhere - S < weight - lies in an allocated brick
    host_s, host_w = dense_s.cpu().numpy(), dense_w.cpu().numpy()
    band = S.bricks_holding(host_s[..., 0] < host_w)
    assert not (band & ~marked).any()


def test_mark_ors_and_wrapper_refusals(hip):
    case = S.MARK_CASES[0]
    r = S.reference(*case)
    views, depth, rgb, kw = _groups(hip, r, case[3])[0]
    bdims = hip.brick_dims(r["dims"])
    args = (r["origin"], r["voxel"], r["dims"], r["trunc"])
    marks = torch.zeros(bdims[::-1], dtype=torch.uint8, device="cuda")
    one = hip.tsdf_bricks_mark(views[:1], depth[:1], *args, marks, **dict(kw, n_consistent=None, min_consistent=0)).clone()
    both = hip.tsdf_bricks_mark(views[1:], depth[1:], *args, marks, **dict(kw, n_consistent=None, min_consistent=0))
    whole = hip.tsdf_bricks_mark(views, depth, *args, torch.zeros_like(marks), **dict(kw, n_consistent=None, min_consistent=0))
    assert torch.equal(both, whole) and bool((one <= both).all()) and 0 < int(one.sum()) <= int(both.sum())
    for bad in (dict(marks=marks[:-1]), dict(marks=marks.int()), dict(marks=marks.cpu()), dict(depth=depth[:2])):
        a = dict(dict(depth=depth, marks=torch.zeros_like(marks)), **bad)
        with pytest.raises(hip.MnerfError):
            hip.tsdf_bricks_mark(views, a["depth"], *args, a["marks"])
    table, bricks, count = hip.tsdf_bricks_table(both, bdims)
    n = int(count.cpu())
    sums, weight = torch.zeros(n, 512, 4, device="cuda"), torch.zeros(n, 512, device="cuda")
    for bad in (dict(n_bricks=n + 1), dict(sums=sums[:-1]), dict(weight=weight.double()), dict(bricks=bricks[:-1]), dict(bricks=bricks.long())):
        a = dict(dict(bricks=bricks, n_bricks=n, sums=sums, weight=weight), **bad)
        with pytest.raises(hip.MnerfError):
            hip.tsdf_integrate_sparse(views, depth, rgb, *args, a["bricks"], a["n_bricks"], a["sums"], a["weight"])
    with pytest.raises(hip.MnerfError):
        hip.tsdf_bricks_table(both, (bdims[0] + 1, bdims[1], bdims[2]))
    torch.cuda.synchronize()
    assert not sums.any() and not weight.any()  # nothing was launched


def test_argument_refusals_precede_any_launch(hip):
    S.assert_refusals(hip)


# ------------------------------------------------------------------------------------------------ b. mesh on an analytic volume
def _dense_mesh(hip, vol, dims):
    s, w = _cuda(vol["sums"]), _cuda(vol["weight"])
    none_v, none_f = torch.empty(0, 8, device="cuda"), torch.empty(0, 3, dtype=torch.int32, device="cuda")
    _, _, counts = hip.tsdf_mesh(s, w, vol["origin"], vol["voxel"], dims, 2.0, none_v, none_f)
    nv, nf = (int(c) for c in counts.cpu())
    v, f = torch.empty(nv, 8, device="cuda"), torch.empty(nf, 3, dtype=torch.int32, device="cuda")
    hip.tsdf_mesh(s, w, vol["origin"], vol["voxel"], dims, 2.0, v, f)
    return v.cpu().numpy(), f.cpu().numpy()


def _sparse_mesh(hip, vol, dims, brick_mask, vertex_rows=None, face_rows=None):
    """the sparse mesher on the test's own bricking of a dense volume (poisoned outside the grid), guarded buffers of exactly the
    given (default: the needed) rows -> vertices, faces, counts"""
    table, bricks = S.table_of(brick_mask)
    n_bricks = len(bricks)
    sums, weight = S.brick_volume(vol["sums"], vol["weight"], table)
    listed = np.full(table.size, -5, np.int32)  # (entries past n_bricks are not read)
    listed[:n_bricks] = bricks
    args = (_cuda(sums), _cuda(weight), _cuda(table), _cuda(listed), n_bricks, vol["origin"], vol["voxel"], dims, 2.0)
    if vertex_rows is None:
        _, _, counts = hip.tsdf_mesh_sparse(*args, torch.empty(0, 8, device="cuda"), torch.empty(0, 3, dtype=torch.int32, device="cuda"))
        vertex_rows, face_rows = (int(c) for c in counts.cpu())
    vbuf, vertices = _guarded(8 * vertex_rows)
    fbuf, faces = _guarded(3 * face_rows, torch.int32, -777)
    need = hip.tsdf_mesh_sparse_workspace_bytes(n_bricks, hip.brick_dims(dims))
    wbuf, ws = _guarded(need, torch.uint8, 77)
    _, _, counts = hip.tsdf_mesh_sparse(*args, vertices.view(-1, 8), faces.view(-1, 3), workspace=ws)
    torch.cuda.synchronize()
    assert _guards_untouched(vbuf, 8 * vertex_rows) and _guards_untouched(fbuf, 3 * face_rows, -777) and _guards_untouched(wbuf, need, 77)
    return vertices.cpu().numpy().reshape(-1, 8), faces.cpu().numpy().reshape(-1, 3), [int(c) for c in counts.cpu()], table


def _needed_bricks(vol, keys=None, dims=None):
    """the mark rule on an analytic volume: NEAR = |d| < 1 in units of the truncation"""
    return S.wanted_bricks(np.abs(vol["sums"][..., 0]) < vol["weight"])


# (12, 11, 13): 2 x 2 x 2 bricks, every axis partial.  (64, 64, 64) with all 512 bricks: exactly 1024 workgroups of 256 points, one
# scan tile; (72, 64, 64) with all 576 bricks: one tile more.
@pytest.mark.parametrize("dims,all_bricks", [((12, 11, 13), True), ((64, 64, 64), False), ((64, 64, 64), True), ((72, 64, 64), True)], ids=str)
def test_mesh_of_the_sphere_is_the_dense_meshers(hip, dims, all_bricks):
    vol, keys = M.sphere_volume(dims), M.sphere_mesh(dims, False, np.float32)
    dense_v, dense_f = _dense_mesh(hip, vol, dims)
    assert np.array_equal(dense_f, keys["faces"]) and len(dense_v) == len(keys["vertices"])  # so the restatement's keys are the GPU's
    brick_mask = np.ones(S.brick_dims(dims)[::-1], bool) if all_bricks else _needed_bricks(vol, keys, dims)
    assert all_bricks or 0 < brick_mask.sum() < brick_mask.size
    vertices, faces, counts, table = _sparse_mesh(hip, vol, dims, brick_mask)
    want_v, want_f = S.renumber(dict(keys, vertices=dense_v, faces=dense_f), dims, table)
    print(f"sparse mesh {dims}: {int(brick_mask.sum())} of {brick_mask.size} bricks, {counts[0]} vertices, {counts[1]} faces")
    assert counts == [len(dense_v), len(dense_f)]
    assert np.array_equal(_bits(vertices), _bits(want_v)) and np.array_equal(faces, want_f)
    area = M.assert_closed_sphere(vertices, faces, vol["voxel"])
    assert 0.9 < area / (4 * np.pi * M.SPHERE_R ** 2) < 1.0
    again = _sparse_mesh(hip, vol, dims, brick_mask)  # two runs: the same bytes
    assert np.array_equal(_bits(again[0]), _bits(vertices)) and np.array_equal(again[1], faces)


def test_a_missing_brick_opens_the_surface_there(hip):
    dims = (64, 64, 64)
    vol, keys = M.sphere_volume(dims), M.sphere_mesh(dims, False, np.float32)
    needed = _needed_bricks(vol, keys, dims)
    owner = keys["vertex_key"][:, 0]
    used = np.zeros_like(needed)
    used[owner // 4096 >> 3, owner // 64 % 64 >> 3, owner % 64 >> 3] = True
    drop = tuple(np.argwhere(used)[len(np.argwhere(used)) // 2])  # a brick that owns vertices
    less = needed.copy()
    less[drop] = False
    full_v, full_f, full_counts, _ = _sparse_mesh(hip, vol, dims, needed)
    vertices, faces, counts, table = _sparse_mesh(hip, vol, dims, less)
    assert 0 < counts[0] < full_counts[0] and 0 < counts[1] < full_counts[1]
    und, forward, backward = M.edge_uses(faces)
    assert (forward <= 1).all() and (backward <= 1).all() and ((forward + backward) == 1).any()  # open, and nowhere doubled
    assert len(np.unique(faces)) == len(vertices)
    # no triangle uses a point of the dropped brick: every vertex lies on an edge between two voxel centres outside it
    lo = np.array(vol["origin"]) + (np.array(drop[::-1]) * 8 + 0.5) * vol["voxel"]
    hi = lo + 7 * vol["voxel"]
    p = vertices[:, :3].astype(np.float64)
    assert not ((p > lo + 1e-6) & (p < hi - 1e-6)).all(1).any()
    # what remains is the full mesh's: the same triangles by position
    rows = {tuple(full_v[f, :3].reshape(-1)) for f in full_f}
    assert all(tuple(vertices[f, :3].reshape(-1)) in rows for f in faces)


def test_capacities_cut_the_rows_not_the_counts(hip):
    dims = (12, 11, 13)
    vol = M.sphere_volume(dims)
    mask = np.ones((2, 2, 2), bool)
    full_v, full_f, counts, _ = _sparse_mesh(hip, vol, dims, mask)
    half = (counts[0] // 2, counts[1] // 2)
    part_v, part_f, part_counts, _ = _sparse_mesh(hip, vol, dims, mask, *half)  # (guards asserted)
    assert part_counts == counts and half[0] > 0 and half[1] > 0
    assert np.array_equal(_bits(part_v), _bits(full_v[:half[0]])) and np.array_equal(part_f, full_f[:half[1]])
    over = _sparse_mesh(hip, vol, dims, mask, counts[0] + 7, counts[1] + 5)
    assert over[2] == counts and np.array_equal(over[1][:counts[1]], full_f) and (over[1][counts[1]:] == -777).all()
    assert (over[0][counts[0]:] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------ c. fusion.mesh
def _same_mesh(a, b):
    """two meshes on the device: the same vertex rows and triangles, bit for bit, in any order"""
    if a[0].shape != b[0].shape or a[1].shape != b[1].shape:
        return False
    ca, cb = S.canonical(a[0].cpu().numpy(), a[1].cpu().numpy()), S.canonical(b[0].cpu().numpy(), b[1].cpu().numpy())
    return np.array_equal(ca[0], cb[0]) and np.array_equal(ca[1], cb[1])


def _same_bytes(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))
                                    for x, y in zip(a, b))


@pytest.fixture(scope="module")
def scene5(hip):
    k, h, w = 5, 24, 32
    s = F.scene(k, h, w, False)
    return _views(hip, s["cams"]), _cuda(s["depth"]), _cuda(M.scene_colours(k, h, w)), (h, w)


def test_fusion_mesh_sparse_is_the_dense_mesh_reordered(hip, scene5, monkeypatch):
    from matchnerf_amd import fusion
    views, depth, rgb, hw = scene5
    copies = []
    to_host = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **k: (copies.append(1), to_host(t, *a, **k))[1])
    dense = fusion.mesh(views, depth, None, rgb, hw, False, resolution=48)
    n_dense, copies[:] = len(copies), []
    sparse = fusion.mesh(views, depth, None, rgb, hw, False, resolution=48, sparse=True)
    n_sparse = len(copies)
    monkeypatch.undo()
    assert n_sparse == n_dense + 1, (n_dense, n_sparse)  # the brick count
    assert dense[1].shape[0] > 500 and _same_mesh(dense, sparse) and not torch.equal(dense[1], sparse[1])
    assert _same_bytes(sparse, fusion.mesh(views, depth, None, rgb, hw, False, resolution=48, sparse=True))
    assert _same_bytes(dense, fusion.mesh(views, depth, None, rgb, hw, False, resolution=48, sparse=False))
    # no consistency pass, opacity, explicit bounds, 20 views in two groups
    k, (h, w) = 20, hw
    s = F.scene(k, h, w, True)
    views, depth, rgb = _views(hip, s["cams"]), _cuda(s["depth"]), _cuda(M.scene_colours(k, h, w))
    args = dict(bounds=((-0.9, -0.8, -0.9), (0.9, 0.8, 0.3)), voxel=0.0375, trunc=0.15, min_weight=3, consistency=False)
    dense = fusion.mesh(views, depth, torch.ones_like(depth), rgb, hw, True, **args)
    sparse = fusion.mesh(views, depth, torch.ones_like(depth), rgb, hw, True, sparse=True, **args)
    assert dense[1].shape[0] > 500 and _same_mesh(dense, sparse)
    # a first guess that is too small: one more run of the mesher, the same mesh
    monkeypatch.setattr(fusion, "SPARSE_GUESS_ROWS", 0)
    assert sparse[0].shape[0] > 1024
    assert _same_bytes(sparse, fusion.mesh(views, depth, torch.ones_like(depth), rgb, hw, True, sparse=True, **args))


def test_fusion_mesh_sparse_with_finishing_decimation_and_texture(hip, scene5):
    import mesh_decimate_helpers as D
    from matchnerf_amd import fusion
    views, depth, rgb, hw = scene5
    args = dict(resolution=48, smooth=2, min_component_fraction=0.02, decimate=2, texture=4)
    got = fusion.mesh(views, depth, None, rgb, hw, False, sparse=True, **args)
    assert len(got) == 4 and _same_bytes(got, fusion.mesh(views, depth, None, rgb, hw, False, sparse=True, **args))  # deterministic
    dense = fusion.mesh(views, depth, None, rgb, hw, False, **args)
    assert got[0].shape == dense[0].shape and got[1].shape == dense[1].shape and got[2].shape == dense[2].shape and got[3].shape == dense[3].shape
    assert got[1].shape[0] > 50 and int(got[1].min()) >= 0 and int(got[1].max()) < got[0].shape[0] and bool(torch.isfinite(got[0]).all())
    # decimation alone: one vertex per occupied cell in ascending cell order, so the rows pair up; the float64 sums run in another
    # order, so positions agree as the dense test's gate has it (an ulp), not bit for bit
    got = fusion.mesh(views, depth, None, rgb, hw, False, sparse=True, resolution=48, decimate=2)
    dense = fusion.mesh(views, depth, None, rgb, hw, False, resolution=48, decimate=2)
    assert got[0].shape == dense[0].shape and got[1].shape == dense[1].shape
    apart = D.one_ulp_apart(got[0][:, :3].cpu().numpy(), dense[0][:, :3].cpu().numpy())
    print(f"sparse decimate=2: {got[0].shape[0]} vertices, {got[1].shape[0]} triangles, "
          f"{int((_bits(got[0].cpu().numpy()) != _bits(dense[0].cpu().numpy())).sum())} words differ from the dense path's")
    assert apart.all()


def test_a_grid_the_dense_path_refuses(hip):
    """201 million voxels (1024 x 1024 x 192; the dense mesher stops at 178 956 970) around the scene of 24 x 32 maps: it fills a
    corner of the box, so a few thousand bricks are allocated"""
    from matchnerf_amd import fusion
    k, h, w = 3, 24, 32
    s = F.scene(k, h, w, False)
    views, depth, rgb = _views(hip, s["cams"]), _cuda(s["depth"]), _cuda(M.scene_colours(k, h, w))
    voxel = 1.0 / 64
    bounds = ((-8.0, -8.0, -2.0), (8.0, 8.0, 1.0))
    dims = (1024, 1024, 192)
    assert hip.tsdf_mesh_workspace_bytes(dims) == -1
    with pytest.raises(ValueError, match="or pass sparse=True"):
        fusion.mesh(views, depth, None, rgb, (h, w), False, bounds=bounds, voxel=voxel, consistency=False)
    # the brick count, before the volume is allocated
    marks = torch.zeros(hip.brick_dims(dims)[::-1], dtype=torch.uint8, device="cuda")
    hip.tsdf_bricks_mark(views, depth, bounds[0], voxel, dims, 4 * voxel, marks, legacy=False)
    n_bricks = int(marks.sum())
    print(f"1024 x 1024 x 192: {n_bricks} of {marks.numel()} bricks")
    assert 0 < n_bricks < 20000 < hip.MAX_BRICKS
    vertices, faces = fusion.mesh(views, depth, None, rgb, (h, w), False, bounds=bounds, voxel=voxel, consistency=False, sparse=True)
    assert faces.shape[0] > 10000 and int(faces.min()) >= 0 and int(faces.max()) < vertices.shape[0]
    assert len(torch.unique(faces)) == vertices.shape[0] and bool(torch.isfinite(vertices).all())
    p = vertices[:, :3].double().cpu().numpy()
    assert (p.min(0) >= np.array(bounds[0])).all() and (p.max(0) <= np.array(bounds[1])).all()
    lo, hi = np.array([-0.4, -0.3, -0.6]), np.array([0.3, 0.35, 0.0])
    to_box = np.where(((p >= lo) & (p <= hi)).all(1), np.minimum(p - lo, hi - p).min(1), np.linalg.norm(np.maximum(np.maximum(lo - p, p - hi), 0), axis=1))
    assert (np.minimum(np.abs(p[:, 2]), to_box) < 4 * voxel).mean() > 0.9  # within the truncation of the plane or the box


# ------------------------------------------------------------------------------------------------ d. the module and the coach
def test_export_mesh_sparse_on_the_synthetic_model(hip):
    from test_fusion_gpu import LOOSE, _model
    opt, model, batch, calls = _model("nonlegacy")
    with torch.no_grad():
        with pytest.raises(ValueError, match="sparse"):
            model.export_mesh(batch, views="sources", resolution=48, sparse="yes", **LOOSE)
        assert calls == []  # refused before the encoder ran
        dense = model.export_mesh(batch, views="sources", resolution=48, **LOOSE)
        sparse = model.export_mesh(batch, views="sources", resolution=48, sparse=True, **LOOSE)
    assert len(sparse) == 1 and sparse[0][1].dtype == torch.int32
    print(f"export_mesh(sparse=True) on the synthetic model: {sparse[0][0].shape[0]} vertices, {sparse[0][1].shape[0]} faces")
    assert _same_mesh(dense[0], sparse[0])


def test_coach_export_geometry_takes_the_option(tmp_path, monkeypatch):
    from test_fusion_gpu import _coach
    loose = ["--nerf.export_geometry=sources", "--nerf.fuse_px_tol=64", "--nerf.fuse_rel_tol=0.9", "--nerf.fuse_min_opacity=0.01",
             "--nerf.fuse_min_views=1", "--nerf.export_mesh", "--nerf.mesh_resolution=48"]
    c = _coach(tmp_path, monkeypatch, *loose)
    written = c.export_geometry()
    before = [open(p, "rb").read() for p in written["dtu"]]
    dense = M.read_ply(written["dtu"][1])
    c.opts.nerf.mesh_sparse = True
    assert c.export_geometry() == written
    xyz, rgb, faces = M.read_ply(written["dtu"][1])
    assert open(written["dtu"][0], "rb").read() == before[0]  # the cloud: the same bytes
    assert xyz.shape == dense[0].shape and faces.shape == dense[2].shape and (len(faces) == 0 or faces.max() < len(xyz))
    if len(faces):  # the same surface: the same set of positions
        assert np.array_equal(np.unique(xyz.view(np.uint32), axis=0), np.unique(dense[0].view(np.uint32), axis=0))
    c.opts.nerf.mesh_sparse = "maybe"
    with pytest.raises(ValueError, match="mesh_sparse"):
        c.export_geometry()
    c.opts.nerf.mesh_sparse = False  # without the option: the files of before, byte for byte
    assert c.export_geometry() == written and [open(p, "rb").read() for p in written["dtu"]] == before
