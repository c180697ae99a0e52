"""Mesh decimation without a GPU: the numpy restatement (tests/mesh_decimate_helpers.py) that the GPU tests compare the kernels with,
tested on its own - identity, planes, a cube's corner, the counts - and the host surface: the binding's table, the library's
host-side checks and workspace formula, the refusals of the Python layers that precede any launch."""
import numpy as np
import pytest

import mesh_decimate_helpers as D
import mesh_finish_helpers as H
from matchnerf_amd import fusion, hip

NEW_EXPORTS = ("mnerf_mesh_decimate_workspace_bytes", "mnerf_mesh_decimate")


# ------------------------------------------------------------------------------------------------ the restatement itself
def test_corner_rows_are_the_adjacency_of_the_finishing_helpers():
    for name, (vertices, faces) in H.small_meshes().items():
        want = H.adjacency(faces, len(vertices))
        got = D.corner_rows(faces, len(vertices))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), name
    offsets, corners = D.corner_rows(np.array([[0, 1, 7], [2, -1, 0]]), 3)  # corners out of range join no row
    assert offsets.tolist() == [0, 2, 3, 4] and corners.tolist() == [0, 5, 1, 3]


def test_identity_where_every_vertex_is_alone_in_its_cell():
    vertices, faces, (origin, cell, dims) = D.lattice_strip()
    out = D.decimate(vertices, faces, origin, cell, dims)
    lin = D.cell_index(vertices, origin, cell, dims)
    assert len(np.unique(lin)) == len(vertices) == len(out["vertices"]) and (out["count"] == 1).all()
    order = np.argsort(lin)  # new row r is the old row order[r]: "ascending cell"
    assert np.array_equal(out["vertex_map"][order], np.arange(len(vertices)))
    assert np.array_equal(out["faces"], out["vertex_map"][faces])  # every face kept, in order, with its winding
    # a lone vertex lies on all its planes: A v + b = 0, the minimiser is the vertex - bit for bit after the rounding to fp32
    assert np.array_equal(out["vertices"].view(np.uint32), vertices[order].view(np.uint32))
    assert (out["lam"] > 0).all()


def test_representatives_of_a_flat_patch_lie_in_its_plane():
    vertices, faces = D.plane_patch()  # z = x / 2 + y / 4 + 3 / 8, satisfied EXACTLY by every fp32 row
    for cell in (0.5, 1.0):  # with this origin the fp32 cell index is exact, so every member lies in its cell's box and no clamp acts
        origin = (-1.0 / 128,) * 3
        dims = tuple(int(d) for d in np.floor((vertices[:, :3].max(0) - origin[0]) / cell) + 1)
        out = D.decimate(vertices, faces, origin, cell, dims)
        p = out["centres"] + out["x"]
        residual = np.abs(0.5 * p[:, 0] + 0.25 * p[:, 1] + 0.375 - p[:, 2]) / cell
        print(f"plane, cell {cell:.2f}: {len(p)} representatives, residual {residual.max():.2e} of the cell")
        assert 4 < len(p) < len(vertices) and (out["count"] > 1).any() and residual.max() < 1e-9


def test_representative_of_a_cubes_corner_is_the_corner():
    vertices, faces, corner = D.cube_corner()
    cell = 0.6
    origin = tuple(float(x) for x in (corner - np.array([0.2, 0.25, 0.15]) - cell).astype(np.float32))
    dims = (4, 4, 4)
    out = D.decimate(vertices, faces, origin, cell, dims)
    lin = D.cell_index(vertices, origin, cell, dims)
    row = out["vertex_map"][np.argmin(np.abs(vertices[:, :3] - corner).sum(1))]  # the cell that holds the corner vertex
    assert out["count"][row] == 7 and lin[0] == out["cells"][row]  # the corner and its six neighbours on the three faces
    a = out["A"][row]
    x0 = vertices[0, :3].astype(np.float64) - out["centres"][row]  # the corner as the fp32 row holds it
    eig = np.linalg.eigvalsh(a)
    assert eig[0] > 0.1 * eig[2]  # three mutually orthogonal planes: full rank
    mean_distance = np.linalg.norm(out["mean"][row] - x0)
    bound = D.REG * np.trace(a) / eig[0] * mean_distance  # from x - x0 = lambda (A + lambda I)^-1 (m - x0)
    distance = np.linalg.norm(out["x"][row] - x0)
    print(f"corner: |x - corner| = {distance:.3e} (bound {bound:.3e}), |mean - corner| = {mean_distance:.3e}, cell {cell}")
    assert distance <= bound * (1 + 1e-9) and bound < 0.01 * mean_distance and distance < mean_distance
    assert np.abs(out["vertices"][row, :3] - vertices[0, :3]).max() < 2 * bound


@pytest.mark.parametrize("name", list(H.small_meshes()))
def test_counts_boxes_and_distinct_triangles(name):
    vertices, faces = H.small_meshes()[name]
    edge = D.mean_edge(vertices, faces)
    for factor in (1.5, 3.0, 8.0):
        origin, cell, dims = D.grid_of(vertices, factor * edge)
        out = D.decimate(vertices, faces, origin, cell, dims)
        lin = D.cell_index(vertices, origin, cell, dims)
        assert len(out["vertices"]) == len(np.unique(lin)) == len(out["cells"]) and (lin >= 0).all(), (name, factor)
        assert np.array_equal(out["cells"][out["vertex_map"]], lin)
        assert (np.abs(out["x"]) <= out["half"]).all()  # the closed box of the cell, before the rounding to fp32
        ulp = np.spacing(np.abs(out["vertices"][:, :3]).astype(np.float32)).astype(np.float64)
        assert (np.abs(out["vertices"][:, :3].astype(np.float64) - out["centres"]) <= out["half"] + ulp).all()
        f = out["faces"]
        assert ((f >= 0) & (f < len(out["vertices"]))).all()
        assert (f[:, 0] != f[:, 1]).all() and (f[:, 1] != f[:, 2]).all() and (f[:, 0] != f[:, 2]).all()
        assert len(np.unique(np.sort(f, 1), axis=0)) == len(f) <= len(faces)
        assert np.isfinite(out["vertices"]).all() and not out["vertices"][:, 7].any()
    origin, cell, dims = D.grid_of(vertices, 4.0 * H.extent_of(vertices))  # one cell: one vertex, the means, no triangle
    out = D.decimate(vertices, faces, origin, cell, dims)
    assert dims == (1, 1, 1) and len(out["vertices"]) == 1 and len(out["faces"]) == 0 and not out["vertex_map"].any()
    assert np.allclose(out["vertices"][0, 3:7], vertices[:, 3:7].astype(np.float64).mean(0), rtol=1e-6)


def test_dropped_rows_and_duplicates_of_both_orientations():
    vertices, faces, origin, cell, dims = D.dropped_case()
    out = D.decimate(vertices, faces, origin, cell, dims)
    assert out["vertex_map"].tolist() == [0, 1, 2, 0, 1, 2, -1, 3]
    assert out["faces"].tolist() == [[0, 1, 2], [1, 2, 3]]
    assert np.isfinite(out["vertices"]).all()


# ------------------------------------------------------------------------------------------------ the host surface
def test_signature_table_and_sources_name_the_decimation():
    assert all(name in hip.SIGNATURES for name in NEW_EXPORTS)
    lib = hip.load()
    assert all(hasattr(lib, name) for name in NEW_EXPORTS)
    from helpers import read_header
    from matchnerf_amd.csrc import build
    assert "mesh_finish.hip" in build.SOURCES  # the file that holds mnerf_mesh_decimate
    assert hip.DECIMATE_REG == 1.0 / read_header().constants["MNERF_DECIMATE_REG_INV"] == D.REG == 1e-3


def test_refusals_and_the_workspace_formula_need_no_gpu():
    D.assert_refusals(hip)
    assert hip.mesh_decimate_workspace_bytes(521, 1038, (7, 9, 5)) == D.workspace_bytes(521, 1038, (7, 9, 5)) > 0
    assert hip.mesh_decimate_workspace_bytes(0, 0, (1, 1, 1)) == 0 and hip.mesh_decimate_workspace_bytes(8, 4, (1 << 11, 1 << 10, 1 << 10)) == -1


def test_python_layers_refuse_before_any_launch():
    import torch
    vertices, faces = (torch.from_numpy(a) for a in H.fan())
    adjacency = tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in D.corner_rows(H.fan()[1], 41))
    with pytest.raises(hip.MnerfError):  # host tensors: there is no CPU path
        hip.mesh_decimate(vertices, faces, adjacency, (0.0, 0.0, 0.0), 1.0, (2, 2, 2))
    anything = object()  # not even looked at
    for cell in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite and >= 0"):
            fusion.finish(anything, anything, decimate_cell=cell)
        with pytest.raises(ValueError, match="finite and >= 0"):
            fusion.decimate(anything, anything, cell)
        with pytest.raises(ValueError, match="finite and >= 0"):
            fusion.mesh([], anything, None, anything, (4, 4), False, decimate=cell)
    with pytest.raises(ValueError):
        fusion.decimate(anything, anything, 0.0)
    with pytest.raises(ValueError, match="go together"):
        fusion.decimate(anything, anything, 1.0, origin=(0.0, 0.0, 0.0))
    assert fusion.finish(anything, anything, decimate_cell=0.0, decimate_origin=None, decimate_dims=None) == (anything, anything)
    from matchnerf_amd.matchnerf import MatchNeRF
    assert "decimate" in MatchNeRF.MESH_ARGS
