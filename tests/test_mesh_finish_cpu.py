"""Mesh finishing without a GPU: the PLY writer with normals, the binding's table, the library's host-side checks, and the sanity of
the numpy restatement (tests/mesh_finish_helpers.py) that the GPU tests compare the kernels with."""
import numpy as np
import pytest

import mesh_finish_helpers as H
import mesh_helpers as M
from matchnerf_amd import fusion, hip

NEW_EXPORTS = ("mnerf_mesh_finish_workspace_bytes", "mnerf_mesh_adjacency", "mnerf_mesh_components", "mnerf_mesh_compact",
               "mnerf_mesh_smooth", "mnerf_mesh_normals")


def test_signature_table_names_the_six_exports():
    assert all(name in hip.SIGNATURES for name in NEW_EXPORTS)
    assert hip.EXPORTS[-6:] == NEW_EXPORTS  # the header's order
    lib = hip.load()
    assert all(hasattr(lib, name) for name in NEW_EXPORTS)


def test_refusals_and_the_workspace_formula_need_no_gpu():
    H.assert_refusals(hip)


def test_write_ply_with_normals_round_trips(tmp_path):
    vertices, faces = H.degenerate()
    normals = H.normals(vertices, faces, H.adjacency(faces, len(vertices)), np.float32)
    path = tmp_path / "n.ply"
    assert fusion.write_ply(str(path), vertices, faces, normals) == len(vertices)
    xyz, nrm, rgb, tri = H.read_ply(path)
    assert np.array_equal(xyz, vertices[:, :3]) and np.array_equal(nrm, normals[:, :3]) and np.array_equal(tri, faces)
    assert np.array_equal(rgb, np.rint(vertices[:, 4:7] * 255.0).astype(np.uint8))
    assert b"property float z\nproperty float nx\nproperty float ny\nproperty float nz\nproperty uchar red" in path.read_bytes()
    # a point cloud with normals, and the refusal of normals of another length
    fusion.write_ply(str(path), vertices, None, normals)
    assert H.read_ply(path)[3] is None and np.array_equal(H.read_ply(path)[1], normals[:, :3])
    with pytest.raises(ValueError, match="normals"):
        fusion.write_ply(str(path), vertices, faces, normals[:-1])


def test_write_ply_without_normals_is_the_file_of_the_old_signature(tmp_path):
    vertices, faces = H.fan()
    a, b, c = tmp_path / "a.ply", tmp_path / "b.ply", tmp_path / "c.ply"
    fusion.write_ply(str(a), vertices, faces)
    fusion.write_ply(str(b), vertices, faces, None)
    fusion.write_ply(str(c), vertices, faces=faces, normals=None)
    assert a.read_bytes() == b.read_bytes() == c.read_bytes()
    xyz, rgb, tri = M.read_ply(a)  # the reader of the mesh export: float xyz + uchar rgb + the face list, nothing else
    assert np.array_equal(xyz, vertices[:, :3]) and np.array_equal(tri, faces)
    assert H.read_ply(a)[1] is None
    fusion.write_ply(str(a), vertices)
    fusion.write_ply(str(b), vertices, None, None)
    assert a.read_bytes() == b.read_bytes() and M.read_ply(a)[2] is None


def test_finish_with_nothing_asked_for_returns_its_inputs():
    vertices, faces = object(), object()  # not even looked at
    assert fusion.finish(vertices, faces) == (vertices, faces)
    assert fusion.finish(vertices, faces, min_component=0, min_component_fraction=0.0, smooth=0)[0] is vertices


# ------------------------------------------------------------------------------------------------ the restatement's own sanity
def test_restatement_adjacency_rows_and_classes():
    for name, (vertices, faces) in H.small_meshes().items():
        offsets, corners, vclass = H.adjacency(faces, len(vertices))
        flat = faces.reshape(-1)
        assert offsets[0] == 0 and offsets[-1] == flat.size and sorted(corners.tolist()) == list(range(flat.size)), name
        for v in (0, len(vertices) // 2, len(vertices) - 1):
            row = corners[offsets[v]:offsets[v + 1]]
            assert (flat[row] == v).all() and (np.diff(row) > 0).all() and len(row) == (flat == v).sum(), (name, v)
    classes = {name: np.bincount(H.adjacency(f, len(v))[2], minlength=2).tolist() for name, (v, f) in H.small_meshes().items()}
    assert classes["sphere"][H.BOUNDARY] == 0 and classes["sphere24"][H.BOUNDARY] == 0 and classes["two_spheres"][H.BOUNDARY] == 0
    assert classes["sphere_open"] == [42, 521 - 42] and len(H.sphere((12, 11, 13), True)[0]) == 521
    assert classes["fan"] == [40, 1] and classes["non_manifold"] == [4, 0] and classes["strip5000"] == [5002, 0]
    assert classes["degenerate"] == [7, 0]
    # the boundary class is the open border: the vertices of the edges that one triangle uses
    vertices, faces, _ = H.sphere((12, 11, 13), True)
    und, forward, backward = M.edge_uses(faces)
    border = np.zeros(len(vertices), bool)
    border[und[forward + backward == 1].reshape(-1)] = True
    assert np.array_equal(H.adjacency(faces, len(vertices))[2] == H.BOUNDARY, border)


def test_restatement_valence_on_the_spheres():
    for dims, open_octant in (((12, 11, 13), False), ((12, 11, 13), True), ((24, 24, 24), False)):
        vertices, faces, _ = H.sphere(dims, open_octant)
        lengths = np.diff(H.adjacency(faces, len(vertices))[0])
        assert 2 <= lengths.min() and lengths.max() <= 10, (dims, open_octant, lengths.min(), lengths.max())


def test_restatement_components_of_the_two_spheres():
    vertices, faces = H.two_spheres()
    labels, keep, count = H.components(faces, len(vertices))
    roots = np.unique(labels)
    assert len(roots) == 2 and keep.all() and (labels <= np.arange(len(vertices))).all() and (labels[roots] == roots).all()
    small, big = sorted(int(count[r]) for r in roots)
    assert small + big == len(faces) and 0 < small < big // 4
    # between the two sizes: exactly the large sphere, a closed surface of its own
    labels, keep, _ = H.components(faces, len(vertices), min_triangles=(small + big) // 2)
    kept_v, kept_f = H.compact(vertices, faces, keep)
    assert len(kept_f) == big and np.array_equal(kept_v, vertices[keep.astype(bool)])
    und, forward, backward = M.edge_uses(kept_f)
    assert (forward == 1).all() and (backward == 1).all() and len(kept_v) - len(und) + len(kept_f) == 2
    assert len(np.unique(kept_f)) == len(kept_v)
    assert np.array_equal(H.components(faces, len(vertices), min_fraction=0.5)[1], keep)
    assert not H.components(faces, len(vertices), min_triangles=big + 1)[1].any()
    # other meshes: one component each, an unreferenced vertex is its own
    assert len(np.unique(H.components(H.strip(5002, 11)[1], 5002)[0])) == 1
    assert H.components(H.degenerate()[1], 7)[0].tolist() == [0, 0, 0, 0, 0, 0, 6]
    assert len(np.unique(H.components(H.strip(257, None, True)[1], 257)[0])) > 4


def test_restatement_smoothing_and_normals_behave():
    noisy, faces, voxel = H.noisy_sphere((12, 11, 13))
    adj = H.adjacency(faces, len(noisy))
    before = H.radial_rms(noisy, voxel)
    after = H.radial_rms(H.smooth(noisy, faces, adj, 10), voxel)
    e32 = H.position_distance(H.smooth(noisy, faces, adj, 10, dtype=np.float32), H.smooth(noisy, faces, adj, 10), H.extent_of(noisy))
    print(f"radial rms {before:.3f} -> {after:.3f} voxel; fp32 restatement after 10 rounds {e32:.2e} of the extent")
    assert 0.25 < before < 0.35 and after < 0.5 * before and e32 < 1e-6
    assert np.array_equal(H.smooth(noisy, faces, adj, 0), noisy[:, :3].astype(np.float64))
    vertices, faces, _ = H.sphere((12, 11, 13))
    adj = H.adjacency(faces, len(vertices))
    n64, n32 = H.normals(vertices, faces, adj), H.normals(vertices, faces, adj, np.float32)
    radial = vertices[:, :3] - np.array(M.SPHERE_C)
    assert ((n64[:, :3] * radial).sum(1) > 0).all() and np.allclose(np.linalg.norm(n64[:, :3], axis=1), 1.0, atol=1e-12)
    assert max(H.normal_distance(n32, n64)) < 1e-5
    area = 0.5 * np.linalg.norm(np.cross(radial[faces[:, 1]] - radial[faces[:, 0]], radial[faces[:, 2]] - radial[faces[:, 0]]), axis=1).sum()
    assert abs(n64[:, 3].sum() - area) < 1e-6 * area  # the thirds add up to the surface
    vertices, faces = H.degenerate()
    n = H.normals(vertices, faces, H.adjacency(faces, 7))
    assert not n[4:].any() and np.isfinite(n).all() and (np.abs(np.linalg.norm(n[:4, :3], axis=1) - 1) < 1e-12).all()
