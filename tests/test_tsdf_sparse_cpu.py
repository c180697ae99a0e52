"""The brick-sparse TSDF volume without a GPU: the restatement of tests/tsdf_sparse_helpers.py pinned by the property the feature
rests on - a dense volume zeroed outside the bricks the mark rule asks for meshes to the SAME vertices and faces, bit for bit -, the
renumbering between the two orders, and the host side: the ABI additions, every argument refusal, the workspace formulas, the
option, the refusals of fusion.mesh(sparse=True) that need no device."""
import os

import numpy as np
import pytest
import torch

import mesh_helpers as M
import tsdf_sparse_helpers as S
from helpers import REPO, read_header
from matchnerf_amd import fusion, hip, options
from matchnerf_amd.csrc import build

NEW_EXPORTS = ("mnerf_tsdf_bricks_mark", "mnerf_tsdf_bricks_table_workspace_bytes", "mnerf_tsdf_bricks_table",
               "mnerf_tsdf_integrate_sparse", "mnerf_tsdf_mesh_sparse_workspace_bytes", "mnerf_tsdf_mesh_sparse")


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("case", list(S.CPU_CASES), ids=lambda c: "-".join(str(x) for x in c))
def test_masking_to_the_marked_bricks_leaves_the_mesh_identical(case):
    """fp32 throughout, as the device: NEAR, the dilated brick set, the volume zeroed outside it, the mesher"""
    r = S.reference(*case)
    bricks = S.wanted_bricks(r["near32"])
    assert bricks.shape == S.brick_dims(r["dims"])[::-1]
    min_weight = S.min_weight_of(case[0])
    dense = M.mesh(r["sums32"], r["weight32"], r["origin"], r["voxel"], min_weight, np.float32)
    masked = M.mesh(*S.mask_volume(r["sums32"], r["weight32"], bricks), r["origin"], r["voxel"], min_weight, np.float32)
    assert (int(bricks.sum()), bricks.size, len(dense["vertices"]), len(dense["faces"])) == S.CPU_CASES[case], case
    print(f"sparse {case}: {int(bricks.sum())} of {bricks.size} bricks, {len(dense['vertices'])} vertices, {len(dense['faces'])} faces, "
          f"{int(r['near32'].sum())} NEAR voxels, {int((r['near32'] != r['near']).sum())} differ from float64, {int(r['unsure'].sum())} unsure")
    assert len(dense["faces"]) > 100
    assert np.array_equal(masked["vertices"].view(np.uint32), dense["vertices"].view(np.uint32))
    assert np.array_equal(masked["faces"], dense["faces"]) and np.array_equal(masked["vertex_key"], dense["vertex_key"])
    # one brick fewer is NOT enough: the rule is not wider than it has to be everywhere (a brick a triangle's cell reads from)
    used = np.zeros_like(bricks)
    owner = dense["vertex_key"][:, 0]
    nx, ny, nz = r["dims"]
    used[owner // (nx * ny) >> 3, owner // nx % ny >> 3, owner % nx >> 3] = True
    assert used.any() and not (used & ~bricks).any()
    # where float64 and fp32 disagree on NEAR the voxel is one the GPU test leaves out
    assert not ((r["near32"] != r["near"]) & ~r["unsure"]).any()


def test_the_renumbering_is_a_permutation_in_the_stated_order():
    case = (3, 24, 32, False, "plain", True, "fine")
    r = S.reference(*case)
    table, listed = S.table_of(S.wanted_bricks(r["near32"]))
    assert np.array_equal(table.reshape(-1)[listed], np.arange(len(listed))) and (table.reshape(-1) >= 0).sum() == len(listed)
    dense = M.mesh(r["sums32"], r["weight32"], r["origin"], r["voxel"], S.min_weight_of(3), np.float32)
    vertices, faces = S.renumber(dense, r["dims"], table)
    assert vertices.shape == dense["vertices"].shape and faces.shape == dense["faces"].shape
    assert not np.array_equal(faces, dense["faces"])  # another order
    for a, b in zip(S.canonical(vertices, faces), S.canonical(dense["vertices"], dense["faces"])):
        assert np.array_equal(a, b)
    # the same triangles, by position and in the same winding
    assert {tuple(vertices[f, :3].reshape(-1)) for f in faces} == {tuple(dense["vertices"][f, :3].reshape(-1)) for f in dense["faces"]}
    # the bricked layout puts every voxel of the grid where point_of says, and poisons the rest of the partial bricks
    sums, weight = S.brick_volume(r["sums32"], r["weight32"], table)
    assert sums.shape == (len(listed), 512, 4) and weight.shape == (len(listed), 512)
    nx, ny, nz = r["dims"]
    iz, iy, ix = np.unravel_index(np.arange(nx * ny * nz), (nz, ny, nx))
    p = S.point_of(table, iz, iy, ix)
    assert np.array_equal(weight.reshape(-1)[p[p >= 0]], r["weight32"].reshape(-1)[p >= 0])
    assert (weight.reshape(-1) == 3).sum() >= 512 * len(listed) - (p >= 0).sum() > 0


def test_dilation_and_bricks_on_a_single_voxel():
    mask = np.zeros((17, 9, 20), bool)  # nz, ny, nx -> 3 x 2 x 3 bricks
    mask[8, 0, 15] = True  # z at the low face of brick 1, y at the grid's face, x at the high face of brick 1
    got = S.wanted_bricks(mask)
    assert got.shape == (3, 2, 3) and sorted(map(tuple, np.argwhere(got))) == [(0, 0, 1), (0, 0, 2), (1, 0, 1), (1, 0, 2)]
    mask[:] = False
    mask[16, 8, 19] = True  # the last voxel of the grid: nothing beyond it, the bricks below it in z and y (it is their first)
    assert sorted(map(tuple, np.argwhere(S.wanted_bricks(mask)))) == [(1, 0, 2), (1, 1, 2), (2, 0, 2), (2, 1, 2)]
    mask[:] = False
    mask[4, 4, 4] = True  # the middle of a brick: that brick alone
    assert sorted(map(tuple, np.argwhere(S.wanted_bricks(mask)))) == [(0, 0, 0)]


# ------------------------------------------------------------------------------------------------ host side
def test_exports_build_and_abi():
    header = read_header()
    names = [name for _, name, _ in header.prototypes]
    lib = hip.load()
    for name in NEW_EXPORTS:
        assert name in hip.SIGNATURES and name in hip.EXPORTS and name in names and hasattr(lib, name), name
    assert "tsdf_sparse.hip" in build.SOURCES and os.path.exists(os.path.join(build.HERE, "tsdf_sparse.hip"))
    assert header.constants["MNERF_TSDF_BRICK"] == 8 == hip.TSDF_BRICK == S.BRICK
    assert lib.mnerf_abi_version() == 12 == hip.MNERF_ABI_VERSION == header.constants["MNERF_ABI_VERSION"]
    assert len(hip.STRUCTS) == 11 and lib.mnerf_struct_size(11) == -1  # no new struct
    assert hip.brick_dims((47, 43, 57)) == (6, 6, 8) and hip.brick_dims((8, 9, 1)) == (1, 2, 1)


def test_argument_refusals_precede_any_hip_call():
    S.assert_refusals(hip)


def test_option_parses_and_defaults_to_absent():
    opt = options.load_options("configs/test.yaml", verbose=False)
    assert getattr(opt.nerf, "mesh_sparse", None) is None and "mesh_sparse" not in opt.nerf
    cmd = options.parse_arguments(["--nerf.export_geometry=sources", "--nerf.export_mesh", "--nerf.mesh_sparse", "--nerf.mesh_resolution=1024"])
    opt = options.override_options(opt, cmd)
    assert opt.nerf.mesh_sparse is True and opt.nerf.mesh_resolution == 1024
    assert fusion._sparse_flag("nerf.mesh_sparse", opt.nerf.mesh_sparse) is True and fusion._sparse_flag("x", 0) is False
    for bad in ("yes", 2, 0.5, None):
        with pytest.raises(ValueError, match="mesh_sparse"):
            fusion._sparse_flag("nerf.mesh_sparse", bad)
    with open(os.path.join(REPO, "test.py")) as f:  # the script's docstring names it
        assert "--nerf.mesh_sparse" in f.read()


def test_mesh_sparse_refuses_on_the_host(monkeypatch):
    monkeypatch.setattr(fusion, "_sparse_volume_mesh", lambda *a, **k: pytest.fail("the volume was reached"))
    views = [object(), object()]
    depth, rgb = torch.ones(2, 4, 4), torch.zeros(2, 16, 3)
    grid = dict(bounds=((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), voxel=1.0 / 4096, consistency=False)
    with pytest.raises(ValueError, match="smallest decimate that fits is 4"):  # 4096^3 cells; 1366^3 > 2^31 > 1024^3
        fusion.mesh(views, depth, None, rgb, (4, 4), True, sparse=True, decimate=1, **grid)
    with pytest.raises(ValueError, match="smallest decimate that fits is 4"):
        fusion.mesh(views, depth, None, rgb, (4, 4), True, sparse=True, decimate=2.5, **grid)
    with pytest.raises(ValueError, match="sparse='maybe'"):
        fusion.mesh(views, depth, None, rgb, (4, 4), True, sparse="maybe", **grid)
    with pytest.raises(ValueError, match="or pass sparse=True"):  # the dense path's refusal names the way out
        fusion.mesh(views, depth, None, rgb, (4, 4), True, **grid)
    with pytest.raises(ValueError, match="at least 2"):
        fusion.mesh([object()], None, None, None, (4, 4), True, sparse=True)
    fusion._decimate_grid_fits("mesh", (4096, 4096, 4096), 4)  # fits: no refusal
    fusion._decimate_grid_fits("mesh", (1024, 1024, 1024), 1)
