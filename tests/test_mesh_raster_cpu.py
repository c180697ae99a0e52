"""Mesh raster without a GPU: the fill rule and the one-owner guarantee on the numpy restatement (tests/mesh_raster_helpers.py), every
refusal of the library, the float32 restatement against the float64 one - what sizes the GPU's depth and bary gates -, the
borderline share of every GPU case, and the purpose of visibility="mesh" on the restatements."""
import numpy as np
import pytest

import mesh_raster_helpers as R
from matchnerf_amd import fusion, hip

NEW_EXPORTS = ("mnerf_mesh_raster_workspace_bytes", "mnerf_mesh_raster", "mnerf_mesh_shade")
CAM = R.pixel_camera()


def test_signature_table_and_sources_name_the_raster():
    from helpers import read_header
    from matchnerf_amd.csrc import build
    names = [name for _, name, _ in read_header().prototypes]
    lib = hip.load()
    for name in NEW_EXPORTS:
        assert name in hip.SIGNATURES and name in hip.EXPORTS and name in names and hasattr(lib, name), name
    assert "mesh_raster.hip" in build.SOURCES
    for name in ("mesh_raster_workspace_bytes", "mesh_raster", "mesh_shade"):
        assert callable(getattr(hip, name))
    assert callable(fusion.render_mesh) and callable(fusion.mesh_report) and callable(fusion.mesh_depths)


def test_argument_refusals_precede_any_hip_call():
    R.assert_refusals(hip)


def cover_count(vertices, faces, h, w, dtype):
    """how many triangles cover every pixel (legacy centres, CAM)"""
    tri = R.setup(vertices, faces, CAM, dtype)
    t, x, y = R.pairs(tri, h, w, True)
    covered = R.evaluate(tri, t, x.astype(dtype), y.astype(dtype), dtype)[0]
    return np.bincount((y * w + x)[covered], minlength=h * w).reshape(h, w)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("hw", [(24, 32), (37, 53), (1, 1)])
def test_fill_rule_on_the_quad(dtype, hw):
    h, w = hw
    want = R.top_left_set(0, 0, 8, 8, h, w)
    for kind in ("quad", "quad_unwelded"):
        vertices, faces = R.hand_mesh(kind)
        r = R.raster(vertices, faces, CAM, h, w, True, dtype)
        assert np.array_equal(r["face"] >= 0, want) and want.sum() == min(h, 8) * min(w, 8)
        assert np.array_equal(cover_count(vertices, faces, h, w, dtype), want.astype(int))  # no hole on the diagonal, none claimed twice
        assert (r["depth"][want] == 2.0).all() and not r["depth"][~want].any()
        y, x = np.nonzero(want)
        assert (r["face"][want] == np.where(x >= y, 0, 1)).all()  # the diagonal's pixels go to the triangle on their +x side


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_one_owner_on_a_vertex_fan(dtype):
    vertices, faces = R.hand_mesh("fan")
    count = cover_count(vertices, faces, 24, 32, dtype)
    assert count.max() == 1 and count[9, 10] == 1  # the shared vertex sits on a pixel centre
    r = R.raster(vertices, faces, CAM, 24, 32, True, dtype)
    assert set(np.unique(r["face"])) == {-1, 0, 1, 2, 3, 4, 5}
    # every centre strictly inside the ring's polygon is covered: the hexagon's interior, by the even-odd rule in exact integers
    ring = np.array([(16, 9), (14, 15), (5, 16), (3, 9), (6, 2), (15, 3)])
    y, x = np.meshgrid(np.arange(24), np.arange(32), indexing="ij")
    a, b = ring, np.roll(ring, -1, 0)
    cross = (b[:, 0] - a[:, 0])[:, None, None] * (y - a[:, 1, None, None]) - (b[:, 1] - a[:, 1])[:, None, None] * (x - a[:, 0, None, None])
    assert (count[(cross > 0).all(0)] == 1).all() and not count[(cross < 0).any(0)].any()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_one_owner_on_the_shared_edges_of_a_welded_grid(dtype):
    """a jittered grid whose vertices lie on quarter pixels - many centres fall ON edges and vertices - in both windings"""
    rng = np.random.default_rng(5)
    n = 9
    gy, gx = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    pos = np.stack([gx * 3.0 + 2.0, gy * 2.5 + 1.0], -1) + np.where(((gx > 0) & (gx < n - 1) & (gy > 0) & (gy < n - 1))[..., None],
                                                                   rng.integers(-4, 5, (n, n, 2)) / 4.0, 0.0)
    vertices = R.rows(pos.reshape(-1, 2), z=2.0)
    quads = [(j * n + i, j * n + i + 1, (j + 1) * n + i + 1, (j + 1) * n + i) for j in range(n - 1) for i in range(n - 1)]
    faces = []
    for q, (a, b, c, d) in enumerate(quads):
        first, second = ((a, b, c), (a, c, d)) if q % 2 else ((a, b, d), (b, c, d))
        faces += [first, second[::-1] if q % 3 == 0 else second]  # mixed windings
    faces = np.array(faces, np.int32)
    count = cover_count(vertices, faces, 24, 32, dtype)
    want = R.top_left_set(2, 1, 26, 21, 24, 32)  # the grid's outline is the rectangle [2, 26] x [1, 21]
    assert np.array_equal(count, want.astype(int))
    on_edge = 0
    tri = R.setup(vertices, faces, CAM, np.float64)
    t, x, y = R.pairs(tri, 24, 32, True)
    d = R.evaluate(tri, t, x.astype(np.float64), y.astype(np.float64), np.float64)[5]
    on_edge = int(((d == 0).any(1) & (d >= 0).all(1)).sum())
    assert on_edge > 40  # the case does put centres on edges


def test_hand_meshes_on_the_restatement():
    vertices, faces = R.hand_mesh("coincident")
    r = R.raster(vertices, faces, CAM, 24, 32, True)
    assert set(np.unique(r["face"])) == {-1, 0}  # equal depths: the lower index
    vertices, faces = R.hand_mesh("huge")
    assert (R.raster(vertices, faces, CAM, 37, 53, True)["face"] == 0).all()
    vertices, faces = R.hand_mesh("nothing")
    assert (R.raster(vertices, faces, CAM, 24, 32, True)["face"] == -1).all()
    vertices, faces = R.hand_mesh("broken")
    r = R.raster(vertices, faces, CAM, 24, 32, True)
    alone = [R.raster(vertices, faces[[t]], CAM, 24, 32, True)["face"] >= 0 for t in (0, 4)]
    assert np.array_equal(r["face"] == 0, alone[0]) and np.array_equal(r["face"] == 4, alone[1]) and set(np.unique(r["face"])) == {-1, 0, 4}


def test_depth_and_weights_are_perspective_correct():
    """a triangle tilted in depth: 1 / z is affine over the screen, and the weights reproduce the world point"""
    vertices = R.rows([(2, 2), (20, 4), (6, 19)], z=[1.0, 2.0, 4.0])
    faces = np.array([[0, 1, 2]], np.int32)
    r = R.raster(vertices, faces, CAM, 24, 32, True)
    y, x = np.nonzero(r["face"] == 0)
    assert len(x) > 100
    b1, b2 = r["bary"][y, x, 0], r["bary"][y, x, 1]
    p = vertices[:, :3].astype(np.float64)
    world = p[0] + b1[:, None] * (p[1] - p[0]) + b2[:, None] * (p[2] - p[0])
    assert np.abs(world[:, 2] - r["depth"][y, x]).max() < 1e-12
    assert np.abs(world[:, 0] / world[:, 2] - x).max() < 1e-12 and np.abs(world[:, 1] / world[:, 2] - y).max() < 1e-12


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_borderline_share_and_the_float32_restatement(case):
    """the condition of the GPU comparison (at most 1 % of a case's pixels are left out) and what sizes its gates"""
    name, decimated, k, h, w, legacy = case
    frames = R.rastered(*case)
    share = float(np.mean([r["border"].mean() for r in frames]))
    worst_depth = worst_bary = 0.0
    for r in frames:
        keep = ~r["border"]
        assert np.array_equal(r["face32"][keep], r["face"][keep])  # the same winner, the same hit / no-hit
        d, b = R.frame_distance(r["depth32"], r["bary32"], r, keep)
        worst_depth, worst_bary = max(worst_depth, d), max(worst_bary, b)
    hit = float(np.mean([(r["face"] >= 0).mean() for r in frames]))
    print(f"raster {case}: {len(R.mesh_of(*case)['faces'])} triangles, hit {hit:.3f}, borderline {share:.5f}, float32 within {worst_depth:.2e} "
          f"(relative depth) and {worst_bary:.2e} (weights) of float64")
    assert share <= R.BORDERLINE_CAP and hit > 0.3
    assert worst_depth <= R.F32_HEADROOM * R.F32_DEPTH_REL and worst_bary <= R.F32_HEADROOM * R.F32_BARY


@pytest.mark.parametrize("case", [c for c in R.CASES if c[2] == 3], ids=lambda c: "-".join(str(x) for x in c))
def test_shade_float32_restatement_within_the_colour_gate(case):
    name, decimated, k, h, w, legacy = case
    m, frames = R.mesh_of(*case), R.rastered(*case)
    atlas, block = R.atlas_of(*case)
    for cam, r in zip(m["cams"], frames):
        keep = ~r["border"] & (r["face"] >= 0)
        for tex, b in ((None, 0), (atlas, block)):
            want, normal = R.shade(m["vertices"], m["faces"], r["face"], r["bary"], cam, tex, b)
            got, _ = R.shade(m["vertices"], m["faces"], r["face32"], r["bary32"], cam, tex, b, np.float32)
            assert np.abs(got.astype(np.float64) - want)[keep].max() <= R.RGB_GATE
            assert (want[..., 3] == (r["face"] >= 0)).all() and not want[r["face"] < 0].any()
        length = np.linalg.norm(normal[..., :3], axis=-1)
        assert np.abs(length[r["face"] >= 0] - 1).max() < 1e-12 and not normal[r["face"] < 0].any()


def test_atlas_shading_reads_only_the_triangles_own_texels():
    case = ("scene", False, 3, 24, 32, False)
    m, frames = R.mesh_of(*case), R.rastered(*case)
    atlas, block = R.atlas_of(*case)
    owner = R.X.layout(len(m["faces"]), block)["owner"]
    for cam, r in zip(m["cams"], frames):
        poisoned = np.where(np.isin(owner, np.unique(r["face"][r["face"] >= 0]))[..., None], atlas, np.float32(np.nan))
        for dtype in (np.float64, np.float32):
            face, bary = (r["face"], r["bary"]) if dtype is np.float64 else (r["face32"], r["bary32"])
            want, _ = R.shade(m["vertices"], m["faces"], face, bary, cam, atlas, block, dtype)
            got, _ = R.shade(m["vertices"], m["faces"], face, bary, cam, poisoned, block, dtype)
            assert np.isfinite(got).all() and np.array_equal(got, want)


def test_visibility_against_the_mesh_sees_more_of_a_decimated_surface():
    r = R.visibility_shares()
    print(f"decimated plane + box, cells of {R.DECIMATE_CELL} voxels, {len(r['faces'])} triangles: a = 1 on {r['views'][0]:.4f} of the owned texels "
          f"with the views' depth (colour RMS {r['views'][1]:.4f}), {r['mesh'][0]:.4f} with the mesh's (colour RMS {r['mesh'][1]:.4f})")
    assert r["mesh"][0] > r["views"][0]


def test_texture_visibility_is_refused_before_anything_is_launched():
    for call in (lambda: fusion.texture(None, None, [], None, None, None, (4, 4), True, visibility="field"),
                 lambda: fusion.mesh([], None, None, None, (4, 4), True, texture_visibility="both"),
                 lambda: fusion._visibility("x", None)):
        with pytest.raises(ValueError):
            call()
