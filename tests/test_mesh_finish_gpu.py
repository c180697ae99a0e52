"""Mesh finishing on the GPU (matchnerf_amd/csrc/mesh_finish.hip) against the numpy restatement of tests/mesh_finish_helpers.py.

Integer results - offsets, corners, class bytes, labels, keep, the compacted rows (bit for bit), the re-numbered faces, both counts -
are EXACTLY the restatement's on every mesh.  Normals: against float64 arithmetic on the same fp32 rows, per component of n within
max(1e-6, 8 x the fp32 restatement's error) and a alike relative to the largest a (measured: n 1.2e-7 .. 1.7e-7, 3.3e-6 on the
sliver triangles of the 24^3 sphere; a 1.0e-7 .. 1.5e-7; the GPU's figures ARE the fp32 restatement's to the printed digits).
Smoothing: positions after 1 and 10 rounds as a fraction of the mesh's extent within max(1e-6, 8 x the fp32 restatement's error)
(measured: 1.3e-7 .. 2.1e-7 after 1 round, 1.6e-7 .. 3.7e-7 after 10; again the fp32 restatement's own).  Every output buffer
lies between guard regions that must stay untouched."""
import functools

import numpy as np
import pytest
import torch

import fusion_helpers as F
import mesh_finish_helpers as H
import mesh_helpers as M

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINELS = {torch.float32: -777.25, torch.int32: -777, torch.uint8: 0xA5, torch.int64: -777}


@pytest.fixture(scope="module")
def hip():
    from matchnerf_amd import hip as h
    h.load()
    assert torch.cuda.is_available(), "the gpu-marked tests need a GPU"
    return h


class Guarded:
    """n elements between two guard regions"""

    def __init__(self, n, dtype):
        self.n, self.value = n, SENTINELS[dtype]
        self.buf = torch.full((n + 2 * GUARD,), self.value, dtype=dtype, device="cuda")
        self.t = self.buf[GUARD:GUARD + n]

    def untouched(self):
        return bool((self.buf[:GUARD] == self.value).all()) and bool((self.buf[GUARD + self.n:] == self.value).all())


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _adjacency(hip, faces, n_vertices):
    """-> the three device tensors (guards asserted)"""
    out = [Guarded(n_vertices + 1, torch.int32), Guarded(faces.numel(), torch.int32), Guarded(n_vertices, torch.uint8)]
    adj = hip.mesh_adjacency(faces, n_vertices, out=tuple(g.t for g in out))
    torch.cuda.synchronize()
    assert all(g.untouched() for g in out)
    return adj


def _components(hip, faces, n_vertices, min_triangles=0, min_fraction=0.0):
    out = [Guarded(n_vertices, torch.int32), Guarded(n_vertices, torch.uint8)]
    labels, keep = hip.mesh_components(faces, n_vertices, min_triangles, min_fraction, out=tuple(g.t for g in out))
    torch.cuda.synchronize()
    assert all(g.untouched() for g in out)
    return labels, keep


def _compact(hip, vertices, faces, keep, vertex_rows=None, face_rows=None):
    """into guarded buffers of exactly the given rows (default: the input's) -> vertices, faces (numpy, all rows), counts"""
    vertex_rows = vertices.shape[0] if vertex_rows is None else vertex_rows
    face_rows = faces.shape[0] if face_rows is None else face_rows
    v, f = Guarded(8 * vertex_rows, torch.float32), Guarded(3 * face_rows, torch.int32)
    _, _, counts = hip.mesh_compact(vertices, faces, keep, v.t.view(vertex_rows, 8), f.t.view(face_rows, 3))
    torch.cuda.synchronize()
    assert v.untouched() and f.untouched()
    return v.t.cpu().numpy().reshape(-1, 8), f.t.cpu().numpy().reshape(-1, 3), [int(c) for c in counts.cpu()]


def _smooth(hip, vertices, faces, adj, iterations, lam=H.LAMBDA, mu=H.MU):
    out = Guarded(vertices.numel(), torch.float32)
    hip.mesh_smooth(vertices, faces, adj, iterations, lam, mu, out=out.t)
    torch.cuda.synchronize()
    assert out.untouched()
    return out.t.cpu().numpy().reshape(-1, 8)


def _normals(hip, vertices, faces, adj):
    out = Guarded(4 * vertices.shape[0], torch.float32)
    hip.mesh_normals(vertices, faces, adj, out=out.t)
    torch.cuda.synchronize()
    assert out.untouched()
    return out.t.cpu().numpy().reshape(-1, 4)


@functools.lru_cache(maxsize=None)
def _thresholds(name):
    """the component thresholds a mesh is filtered with: between its component sizes where it has several"""
    vertices, faces = H.small_meshes()[name]
    sizes = np.unique(H.components(faces, len(vertices))[2])
    sizes = sizes[sizes > 0]
    return int(sizes[len(sizes) // 2]) if len(sizes) else 1


# ------------------------------------------------------------------------------------------------ integer results, exactly
@pytest.mark.parametrize("name", list(H.small_meshes()))
def test_integer_results_are_the_restatement(hip, name):
    vertices, faces = H.small_meshes()[name]
    n_vertices = len(vertices)
    dv, df = _cuda(vertices), _cuda(faces)
    offsets, corners, vclass = (t.cpu().numpy() for t in _adjacency(hip, df, n_vertices))
    want = H.adjacency(faces, n_vertices)
    assert np.array_equal(offsets, want[0]) and np.array_equal(corners, want[1]) and np.array_equal(vclass, want[2]), name
    min_triangles = _thresholds(name)
    for args in (dict(), dict(min_triangles=min_triangles), dict(min_fraction=0.5), dict(min_triangles=3, min_fraction=0.01),
                 dict(min_triangles=len(faces) + 1)):
        labels, keep = _components(hip, df, n_vertices, **args)
        want_labels, want_keep, _ = H.components(faces, n_vertices, **args)
        assert np.array_equal(labels.cpu().numpy(), want_labels), (name, args)
        assert np.array_equal(keep.cpu().numpy(), want_keep), (name, args)
        got_v, got_f, counts = _compact(hip, dv, df, keep)
        want_v, want_f = H.compact(vertices, faces, want_keep)
        assert counts == [len(want_v), len(want_f)], (name, args, counts)
        assert np.array_equal(_bits(got_v[:counts[0]]), _bits(want_v)) and np.array_equal(got_f[:counts[1]], want_f), (name, args)
        assert (got_v[counts[0]:] == SENTINELS[torch.float32]).all() and (got_f[counts[1]:] == SENTINELS[torch.int32]).all()
    # an arbitrary keep (the compaction does not ask where it comes from): a seeded half of the vertices
    keep = (np.random.default_rng(len(faces)).random(n_vertices) < 0.5).astype(np.uint8)
    got_v, got_f, counts = _compact(hip, dv, df, _cuda(keep))
    want_v, want_f = H.compact(vertices, faces, keep)
    assert counts == [len(want_v), len(want_f)] and np.array_equal(_bits(got_v[:counts[0]]), _bits(want_v))
    kept_first = keep[faces[:, 0]].astype(bool)  # (faces whose other vertices are dropped get the index -1 there)
    assert np.array_equal(got_f[:counts[1], 0], want_f[:, 0]) and np.array_equal(got_f[:counts[1]], np.where(keep[faces[kept_first]] > 0, want_f, -1))


@pytest.mark.parametrize("n_vertices", H.BOUNDARY_SIZES[2:])
def test_strips_across_the_scan_tile_boundary(hip, n_vertices):
    """V one below and one above the 256 x 1024 vertices of one scan tile (the workgroup boundary, 255 and 257, is among the small
    meshes): adjacency, components of many sizes, compaction"""
    vertices, faces = H.strip(n_vertices, None, True)
    dv, df = _cuda(vertices), _cuda(faces)
    got = [t.cpu().numpy() for t in _adjacency(hip, df, n_vertices)]
    want = H.adjacency(faces, n_vertices)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    labels, keep = _components(hip, df, n_vertices, min_triangles=20)
    want_labels, want_keep, _ = H.components(faces, n_vertices, min_triangles=20)
    assert np.array_equal(labels.cpu().numpy(), want_labels) and np.array_equal(keep.cpu().numpy(), want_keep)
    assert 0.2 < want_keep.mean() < 0.95
    got_v, got_f, counts = _compact(hip, dv, df, keep)
    want_v, want_f = H.compact(vertices, faces, want_keep)
    assert counts == [len(want_v), len(want_f)]
    assert np.array_equal(_bits(got_v[:counts[0]]), _bits(want_v)) and np.array_equal(got_f[:counts[1]], want_f)


def _device_two_spheres(hip):
    """the two-sphere volume meshed by hip.tsdf_mesh -> (vertices, faces) on the device; the faces are the restatement's"""
    vol = H.two_sphere_volume()
    nz, ny, nx = vol["weight"].shape
    args = (_cuda(vol["sums"]), _cuda(vol["weight"]), vol["origin"], vol["voxel"], (nx, ny, nz), 2.0)
    _, _, counts = hip.tsdf_mesh(*args, torch.empty(0, 8, device="cuda"), torch.empty(0, 3, dtype=torch.int32, device="cuda"))
    n_vertices, n_faces = (int(c) for c in counts.cpu())
    vertices, faces, _ = hip.tsdf_mesh(*args, torch.empty(n_vertices, 8, device="cuda"), torch.empty(n_faces, 3, dtype=torch.int32, device="cuda"))
    assert np.array_equal(faces.cpu().numpy(), H.two_spheres()[1])
    return vertices, faces


def test_two_spheres_filtered_leave_the_large_one(hip):
    vertices, faces = _device_two_spheres(hip)
    n_vertices = vertices.shape[0]
    host_v, host_f = vertices.cpu().numpy(), faces.cpu().numpy()
    _, _, count = H.components(host_f, n_vertices)
    small, big = sorted(int(c) for c in count[count > 0])
    assert small + big == len(host_f)
    labels, keep = _components(hip, faces, n_vertices, min_triangles=(small + big) // 2)
    want_labels, want_keep, _ = H.components(host_f, n_vertices, min_triangles=(small + big) // 2)
    assert np.array_equal(labels.cpu().numpy(), want_labels) and np.array_equal(keep.cpu().numpy(), want_keep)
    kept_v, kept_f, counts = _compact(hip, vertices, faces, keep)
    assert counts[1] == big and counts[0] == int(want_keep.sum()) and counts[0] < n_vertices
    kept_v, kept_f = kept_v[:counts[0]], kept_f[:counts[1]]
    want_v, want_f = H.compact(host_v, host_f, want_keep)
    assert np.array_equal(_bits(kept_v), _bits(want_v)) and np.array_equal(kept_f, want_f)
    und, forward, backward = M.edge_uses(kept_f)  # exactly the large sphere: closed, consistently wound, every vertex used
    assert (forward == 1).all() and (backward == 1).all() and len(kept_v) - len(und) + len(kept_f) == 2
    assert len(np.unique(kept_f)) == len(kept_v)
    centre, radius = H.TWO_SPHERES["big"]
    assert np.abs(np.linalg.norm(kept_v[:, :3] - np.array(centre), axis=1) - radius).max() < 0.5 * H.TWO_SPHERES["voxel"]
    # min_fraction = 0.5: the same bytes
    _, keep_f = _components(hip, faces, n_vertices, min_fraction=0.5)
    frac_v, frac_f, frac_counts = _compact(hip, vertices, faces, keep_f)
    assert frac_counts == counts and np.array_equal(_bits(frac_v[:counts[0]]), _bits(kept_v)) and np.array_equal(frac_f[:counts[1]], kept_f)
    # above both spheres: nothing
    _, none = _components(hip, faces, n_vertices, min_triangles=big + 1)
    assert _compact(hip, vertices, faces, none)[2] == [0, 0]
    # capacities below the totals cut rows, not counts
    half = (counts[0] // 2, counts[1] // 2)
    part_v, part_f, part_counts = _compact(hip, vertices, faces, keep, *half)  # (guards asserted)
    assert part_counts == counts and half[0] > 0 and half[1] > 0
    assert np.array_equal(_bits(part_v), _bits(kept_v[:half[0]])) and np.array_equal(part_f, kept_f[:half[1]])
    assert _compact(hip, vertices, faces, keep, 0, 0)[2] == counts


# ------------------------------------------------------------------------------------------------ normals
NORMAL_MESHES = ("sphere", "sphere_open", "sphere24", "two_spheres", "fan", "degenerate", "non_manifold")


@pytest.mark.parametrize("name", NORMAL_MESHES)
def test_normals_against_float64_on_the_same_rows(hip, name):
    vertices, faces = H.small_meshes()[name]
    dv, df = _cuda(vertices), _cuda(faces)
    adj = _adjacency(hip, df, len(vertices))
    got = _normals(hip, dv, df, adj)
    host_adj = H.adjacency(faces, len(vertices))
    want, want32 = H.normals(vertices, faces, host_adj), H.normals(vertices, faces, host_adj, np.float32)
    (e_n, e_a), (r_n, r_a) = H.normal_distance(got, want), H.normal_distance(want32, want)
    print(f"normals {name}: n {e_n:.3e} (fp32 restatement {r_n:.3e}), a {e_a:.3e} (fp32 restatement {r_a:.3e})")
    assert np.isfinite(got).all()
    assert e_n < max(1e-6, 8 * r_n) and e_a < max(1e-6, 8 * r_a), (name, e_n, r_n, e_a, r_a)  # every vertex, none left out
    length = np.linalg.norm(got[:, :3].astype(np.float64), axis=1)
    zero = ~want[:, :3].any(1)
    assert not got[zero, :3].any() and (np.abs(length[~zero] - 1) < 1e-6).all()
    if name.startswith("sphere"):
        radial = vertices[:, :3].astype(np.float64) - np.array(M.SPHERE_C)
        assert ((got[:, :3] * radial).sum(1) > 0).all()  # outwards, at every vertex (of the open sphere too)
    if name == "degenerate":  # zero-area triangles only (4, 5), unreferenced (6): exact zeros, the area too
        assert zero.tolist() == [False] * 4 + [True] * 3 and not got[4:].any()


# ------------------------------------------------------------------------------------------------ smoothing
@pytest.mark.parametrize("name", ["sphere", "sphere_open", "sphere24", "two_spheres", "fan"])
def test_smoothing_against_float64(hip, name):
    vertices, faces = H.small_meshes()[name]
    dv, df = _cuda(vertices), _cuda(faces)
    adj = _adjacency(hip, df, len(vertices))
    host_adj = H.adjacency(faces, len(vertices))
    extent = H.extent_of(vertices)
    for iterations in (1, 10):
        got = _smooth(hip, dv, df, adj, iterations)
        want = H.smooth(vertices, faces, host_adj, iterations)
        e32 = H.position_distance(H.smooth(vertices, faces, host_adj, iterations, dtype=np.float32), want, extent)
        err = H.position_distance(got[:, :3], want, extent)
        print(f"smooth {name} x{iterations}: {err:.3e} of the extent (fp32 restatement {e32:.3e})")
        assert err < max(1e-6, 8 * e32), (name, iterations, err, e32)
        assert np.array_equal(_bits(got[:, 3:]), _bits(vertices[:, 3:]))  # w | r g b 0: bit for bit
        boundary = host_adj[2] == H.BOUNDARY
        assert np.array_equal(_bits(got[boundary]), _bits(vertices[boundary]))
        assert (got[~boundary, :3] != vertices[~boundary, :3]).any()
    # plain Laplacian smoothing: mu = 0
    got = _smooth(hip, dv, df, adj, 3, 0.5, 0.0)
    assert H.position_distance(got[:, :3], H.smooth(vertices, faces, host_adj, 3, 0.5, 0.0), extent) < 1e-6


def test_smoothing_of_the_open_sphere_keeps_its_border(hip):
    vertices, faces, _ = H.sphere((12, 11, 13), True)
    dv, df = _cuda(vertices), _cuda(faces)
    adj = _adjacency(hip, df, len(vertices))
    boundary = adj[2].cpu().numpy() == H.BOUNDARY
    assert boundary.sum() == 42 and len(vertices) == 521
    got = _smooth(hip, dv, df, adj, 10)
    assert np.array_equal(_bits(got[boundary]), _bits(vertices[boundary])) and (got[~boundary, :3] != vertices[~boundary, :3]).any()
    assert np.array_equal(_bits(got[:, 3:]), _bits(vertices[:, 3:]))


@pytest.mark.parametrize("dims", [(12, 11, 13), (24, 24, 24)], ids=str)
def test_smoothing_halves_radial_noise(hip, dims):
    noisy, faces, voxel = H.noisy_sphere(dims)
    dv, df = _cuda(noisy), _cuda(faces)
    adj = _adjacency(hip, df, len(noisy))
    before, after = H.radial_rms(noisy, voxel), H.radial_rms(_smooth(hip, dv, df, adj, 10), voxel)
    print(f"radial noise {dims}: {before:.3f} -> {after:.3f} voxel after 10 rounds")
    assert 0.25 < before < 0.35 and after < 0.5 * before


def test_smoothing_zero_rounds_and_in_place(hip):
    noisy, faces, _ = H.noisy_sphere((12, 11, 13))
    dv, df = _cuda(noisy), _cuda(faces)
    adj = _adjacency(hip, df, len(noisy))
    assert np.array_equal(_bits(_smooth(hip, dv, df, adj, 0)), _bits(noisy))
    same = dv.clone()
    assert hip.mesh_smooth(same, df, adj, 0, out=same).data_ptr() == same.data_ptr()
    assert torch.equal(same.view(torch.int32), dv.view(torch.int32))
    for iterations in (1, 4):
        apart = _smooth(hip, dv, df, adj, iterations)
        in_place = dv.clone()
        hip.mesh_smooth(in_place, df, adj, iterations, out=in_place)
        assert np.array_equal(_bits(in_place.cpu().numpy()), _bits(apart)), iterations
    assert torch.equal(dv.view(torch.int32), _cuda(noisy).view(torch.int32))  # out of place: the input is not written


# ------------------------------------------------------------------------------------------------ empty meshes, determinism, refusals
def test_empty_meshes(hip):
    from matchnerf_amd import fusion
    none_v, none_f = torch.empty(0, 8, device="cuda"), torch.empty(0, 3, dtype=torch.int32, device="cuda")
    offsets, corners, vclass = _adjacency(hip, none_f, 0)
    assert offsets.tolist() == [0] and corners.numel() == 0 and vclass.numel() == 0
    assert _compact(hip, none_v, none_f, torch.empty(0, dtype=torch.uint8, device="cuda"))[2] == [0, 0]
    assert fusion.vertex_normals(none_v, none_f).shape == (0, 4)
    out = fusion.finish(none_v, none_f, min_component=3, smooth=2)
    assert out[0].shape == (0, 8) and out[1].shape == (0, 3)
    # vertices without triangles: empty rows, every vertex its own component, zero normals, nothing moves
    vertices = _cuda(H.degenerate()[0])
    adj = _adjacency(hip, none_f, 7)
    assert adj[0].tolist() == [0] * 8 and adj[2].tolist() == [H.BOUNDARY] * 7
    labels, keep = _components(hip, none_f, 7)
    assert labels.tolist() == list(range(7)) and keep.tolist() == [1] * 7
    assert _components(hip, none_f, 7, min_triangles=1)[1].tolist() == [0] * 7
    assert not _normals(hip, vertices, none_f, adj).any()
    assert np.array_equal(_bits(_smooth(hip, vertices, none_f, adj, 2)), _bits(H.degenerate()[0]))
    kept_v, kept_f, counts = _compact(hip, vertices, none_f, _cuda(np.array([1, 0, 1, 1, 0, 0, 1], np.uint8)))
    assert counts == [4, 0] and np.array_equal(_bits(kept_v[:4]), _bits(H.degenerate()[0][[0, 2, 3, 6]]))
    # ... and the triangle total is WRITTEN as 0 (the scan over no element still enqueues its total), not left as it was
    stale = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    hip.mesh_compact(vertices, none_f, _cuda(np.array([1, 0, 1, 1, 0, 0, 1], np.uint8)), counts=stale)
    assert stale.tolist() == [4, 0]


def test_two_runs_give_the_same_bytes(hip):
    from matchnerf_amd import fusion
    vertices, faces = _device_two_spheres(hip)
    small = int(np.unique(H.components(H.two_spheres()[1], vertices.shape[0])[2])[1])
    runs = []
    for _ in range(2):
        v, f = fusion.finish(vertices, faces, min_component=small + 1, smooth=5)
        runs.append((v, f, fusion.vertex_normals(v, f)))
    assert runs[0][0].shape[0] < vertices.shape[0] and runs[0][1].shape[0] == faces.shape[0] - small
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(*runs))
    # finish is its stages: the filter, the adjacency of the RESULT, the smoothing
    host_v, host_f = vertices.cpu().numpy(), faces.cpu().numpy()
    kept_v, kept_f = H.compact(host_v, host_f, H.components(host_f, len(host_v), min_triangles=small + 1)[1])
    assert np.array_equal(runs[0][1].cpu().numpy(), kept_f)
    want = H.smooth(kept_v, kept_f, H.adjacency(kept_f, len(kept_v)), 5)
    assert H.position_distance(runs[0][0][:, :3].cpu().numpy(), want, H.extent_of(kept_v)) < 1e-6
    assert np.array_equal(_bits(runs[0][0][:, 3:].cpu().numpy()), _bits(kept_v[:, 3:]))
    # smoothing alone, and nothing at all
    v, f = fusion.finish(vertices, faces, smooth=1)
    assert f is faces and v.shape == vertices.shape and not torch.equal(v, vertices)
    assert fusion.finish(vertices, faces) == (vertices, faces)


def test_argument_refusals_precede_any_launch(hip):
    H.assert_refusals(hip)
    vertices, faces = (_cuda(x) for x in H.fan())
    n = vertices.shape[0]
    adj = hip.mesh_adjacency(faces, n)
    guards = [Guarded(8 * n, torch.float32), Guarded(4 * n, torch.float32), Guarded(n, torch.int32), Guarded(n, torch.uint8)]
    out_v, out_n, out_l, out_k = (g.t for g in guards)
    wrong = [lambda: hip.mesh_smooth(vertices, faces, adj, -1, out=out_v), lambda: hip.mesh_smooth(vertices, faces, adj, 1, 0.0, out=out_v),
             lambda: hip.mesh_smooth(vertices, faces, adj, 1, 1.5, out=out_v), lambda: hip.mesh_smooth(vertices, faces, adj, 1, 0.5, 0.1, out=out_v),
             lambda: hip.mesh_smooth(vertices, faces, adj, 1, 0.5, float("nan"), out=out_v),
             lambda: hip.mesh_smooth(vertices, faces, (adj[0][:-1], adj[1], adj[2]), 1, out=out_v),
             lambda: hip.mesh_smooth(vertices, faces.long(), adj, 1, out=out_v),
             lambda: hip.mesh_smooth(vertices, faces, adj, 1, out=out_v, workspace=torch.empty(16, dtype=torch.uint8, device="cuda")),
             lambda: hip.mesh_normals(vertices, faces, (adj[0], adj[1][:-1], adj[2]), out=out_n),
             lambda: hip.mesh_normals(vertices.cpu(), faces, adj, out=out_n),
             lambda: hip.mesh_normals(vertices.view(-1)[:-1], faces, adj, out=out_n),
             lambda: hip.mesh_components(faces, n, -1, out=(out_l, out_k)), lambda: hip.mesh_components(faces, n, 0, 1.5, out=(out_l, out_k)),
             lambda: hip.mesh_components(faces, n, 0, float("nan"), out=(out_l, out_k)),
             lambda: hip.mesh_components(faces, n, out=(out_l, out_k.int())),
             lambda: hip.mesh_compact(vertices, faces, out_k[:-1], out_v.view(-1, 8)),
             lambda: hip.mesh_compact(vertices, faces, out_k, out_v.view(-1, 8), counts=torch.zeros(2, dtype=torch.int32, device="cuda")),
             lambda: hip.mesh_adjacency(faces.view(-1)[:-1], n), lambda: hip.mesh_adjacency(faces, -1)]
    for call in wrong:
        with pytest.raises(hip.MnerfError):
            call()
    torch.cuda.synchronize()
    assert all(g.untouched() for g in guards)
    assert all(bool((g.t == g.value).all()) for g in guards)  # and nothing in between was written either


# ------------------------------------------------------------------------------------------------ the host paths
def test_fusion_mesh_applies_finish_to_its_result(hip):
    from matchnerf_amd import fusion
    k, h, w = 5, 24, 32
    s = F.scene(k, h, w, False)
    views, depth, rgb = [hip.make_view(c["extr"], c["intr"], c["near"], c["far"]) for c in s["cams"]], _cuda(s["depth"]), _cuda(M.scene_colours(k, h, w))
    plain = fusion.mesh(views, depth, None, rgb, (h, w), False, resolution=40)
    again = fusion.mesh(views, depth, None, rgb, (h, w), False, resolution=40, min_component=0, min_component_fraction=0.0, smooth=0)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(plain, again))
    # without the new arguments: the mesher's own output - every vertex used, as the mesh export's test asserts it
    assert plain[1].shape[0] > 500 and len(torch.unique(plain[1])) == plain[0].shape[0]
    args = dict(min_component=50, min_component_fraction=0.02, smooth=3, smooth_lambda=0.6, smooth_mu=-0.63)
    got = fusion.mesh(views, depth, None, rgb, (h, w), False, resolution=40, **args)
    want = fusion.finish(*plain, **args)
    assert len(got) == 2 and all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got, want))
    assert got[0].shape == (int(got[1].max()) + 1, 8) and not torch.equal(got[0][:, :3], plain[0][:got[0].shape[0], :3])
    normals = fusion.vertex_normals(*got)
    length = normals[:, :3].norm(dim=1)
    assert normals.shape == (got[0].shape[0], 4) and bool(((length - 1).abs() < 1e-5).logical_or(length == 0).all())


def test_export_mesh_with_normals_on_the_synthetic_model(hip):
    from test_fusion_gpu import LOOSE, _model
    opt, model, batch, calls = _model("nonlegacy")
    with torch.no_grad():
        with pytest.raises(TypeError):
            model.export_mesh(batch, smoothing=1)
        plain = model.export_mesh(batch, views="sources", resolution=48, **LOOSE)
        meshes = model.export_mesh(batch, views="sources", resolution=48, normals=True, min_component_fraction=0.1, smooth=2, **LOOSE)
    assert len(plain) == 1 and len(plain[0]) == 2 and len(meshes) == 1 and len(meshes[0]) == 3
    vertices, faces, normals = meshes[0]
    print(f"export_mesh with normals: {vertices.shape[0]} of {plain[0][0].shape[0]} vertices, {faces.shape[0]} of {plain[0][1].shape[0]} faces")
    assert vertices.shape[1] == 8 and faces.shape[1] == 3 and faces.dtype == torch.int32 and normals.shape == (vertices.shape[0], 4)
    assert vertices.shape[0] <= plain[0][0].shape[0] and faces.shape[0] <= plain[0][1].shape[0]
    assert bool(torch.isfinite(vertices).all()) and bool(torch.isfinite(normals).all())
    assert faces.numel() == 0 or (int(faces.min()) >= 0 and int(faces.max()) < vertices.shape[0])


def test_coach_export_geometry_with_the_finishing_options(tmp_path, monkeypatch):
    from test_fusion_gpu import _coach
    loose = ["--nerf.export_geometry=sources", "--nerf.fuse_px_tol=64", "--nerf.fuse_rel_tol=0.9", "--nerf.fuse_min_opacity=0.01",
             "--nerf.fuse_min_views=1"]
    c = _coach(tmp_path, monkeypatch, *loose, "--nerf.export_mesh", "--nerf.mesh_resolution=48", "--nerf.mesh_min_component=4",
               "--nerf.mesh_min_component_fraction=0.05", "--nerf.mesh_smooth=2", "--nerf.mesh_normals")
    written = c.export_geometry()
    assert list(written) == ["dtu"] and len(written["dtu"]) == 2 and written["dtu"][1].endswith("_mesh.ply")
    header = open(written["dtu"][1], "rb").read(400).split(b"end_header")[0].decode("ascii")
    assert "property float nx\nproperty float ny\nproperty float nz\n" in header
    xyz, normals, rgb, faces = H.read_ply(written["dtu"][1])  # (the reader asserts the header's counts against the body)
    assert normals is not None and faces is not None and np.isfinite(xyz).all()
    assert len(faces) == 0 or (faces.min() >= 0 and faces.max() < len(xyz))
    length = np.linalg.norm(normals.astype(np.float64), axis=1)
    assert ((np.abs(length - 1) < 1e-5) | (length == 0)).all()
    assert M.read_ply(written["dtu"][0])[2] is None  # the cloud next to it: the file of today, no normals
