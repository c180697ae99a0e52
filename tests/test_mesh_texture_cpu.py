"""Mesh texture without a GPU: the layout's guarantees on the numpy restatement (tests/mesh_texture_helpers.py), the host-only atlas
call and every refusal of the library, the reachability of the GPU gate (fp32 restatement against fp64), the borderline share of
every GPU case, the purpose of the feature on the restatement, and the OBJ writer."""
import numpy as np
import pytest

import mesh_decimate_helpers as D
import mesh_texture_helpers as X
from matchnerf_amd import fusion, hip

NEW_EXPORTS = ("mnerf_mesh_texture_atlas", "mnerf_mesh_texture_uv", "mnerf_mesh_texture_accumulate", "mnerf_mesh_texture_resolve")
LAYOUTS = [(t, b) for t in X.LAYOUT_T for b in X.LAYOUT_B]


def test_signature_table_and_sources_name_the_texture():
    from helpers import read_header
    from matchnerf_amd.csrc import build
    names = [name for _, name, _ in read_header().prototypes]
    lib = hip.load()
    for name in NEW_EXPORTS:
        assert name in hip.SIGNATURES and name in hip.EXPORTS and name in names and hasattr(lib, name), name
    assert "mesh_texture.hip" in build.SOURCES
    for name in ("mesh_texture_atlas", "mesh_texture_uv", "mesh_texture_accumulate", "mesh_texture_resolve"):
        assert callable(getattr(hip, name))
    assert callable(fusion.texture) and callable(fusion.write_obj)


@pytest.mark.parametrize("t,b", LAYOUTS)
def test_atlas_size_and_single_ownership(t, b):
    width, height, nbx, nby = X.atlas_size(t, b)
    nb = (t + 1) // 2
    assert nbx * nbx >= nb and (nbx == 0 or (nbx - 1) ** 2 < nb) and nbx * nby >= nb and (nby == 0 or nbx * (nby - 1) < nb)
    assert (width, height) == (nbx * b, nby * b)
    assert hip.mesh_texture_atlas(t, b) == (width, height)  # the host-only call, without a GPU
    lay = X.layout(t, b)
    assert lay["owner"].shape == (height, width)
    counts = np.bincount(lay["owner"][lay["owner"] >= 0], minlength=t)
    # every texel of a used block has exactly one owner (it is a function), every triangle owns its half of a block, and the texels
    # without an owner are exactly those of triangles >= T
    lower, upper = b * (b + 1) // 2, b * (b - 1) // 2
    assert np.array_equal(counts, np.where(np.arange(t) % 2 == 0, lower, upper))
    assert (lay["owner"] < 0).sum() == width * height - counts.sum()
    for p in range(nb):  # each block's texels belong to its two triangles only
        block = lay["owner"][(p // nbx) * b:(p // nbx + 1) * b, (p % nbx) * b:(p % nbx + 1) * b]
        assert set(np.unique(block)) <= {2 * p, 2 * p + 1 if 2 * p + 1 < t else -1}


@pytest.mark.parametrize("t,b", LAYOUTS)
def test_bilinear_fetches_inside_a_uv_triangle_touch_only_its_own_texels(t, b):
    if t == 0:
        assert X.uv(0, b).shape == (0, 3, 2)
        return
    rng = np.random.default_rng(100 * t + b)
    lay, c = X.layout(t, b), X.corners(t, b)
    e1, e2 = c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]
    assert (e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0] > 0).all()  # the UV triangles keep one winding (y down: the stored one)
    assert np.array_equal(c % 1.0, np.full(c.shape, 0.5))  # the corners fall on texel centres
    ab = rng.dirichlet((1.0, 1.0, 1.0), (t, 24))[..., 1:]
    special = np.array([[0, 0], [1, 0], [0, 1], [0.5, 0], [0, 0.5], [0.5, 0.5], [0.25, 0.75], [0.75, 0.25]])  # corners and edge points: exact
    ab = np.concatenate([ab, np.broadcast_to(special, (t, len(special), 2))], 1)
    pts = c[:, None, 0] + ab[..., :1] * e1[:, None] + ab[..., 1:] * e2[:, None]
    fx, fy = pts[..., 0] - 0.5, pts[..., 1] - 0.5
    x0, y0 = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
    ax, ay = fx - x0, fy - y0
    tri = np.arange(t)[:, None]
    touched = 0
    for dx, wx in ((0, 1 - ax), (1, ax)):
        for dy, wy in ((0, 1 - ay), (1, ay)):
            live = wx * wy > 1e-12  # (a random point is farther than that from every texel boundary it does not lie on exactly)
            x, y = x0 + dx, y0 + dy
            assert (x[live] >= 0).all() and (x[live] < lay["W"]).all() and (y[live] >= 0).all() and (y[live] < lay["H"]).all()
            assert np.array_equal(lay["owner"][y[live], x[live]], np.broadcast_to(tri, x.shape)[live])
            touched += int(live.sum())
    assert touched >= t * 32
    # the surface coordinates of the corner texels are the corners, and every texel's lie in the closed triangle
    a, bb = X.bary(b, lay["i"], lay["j"], np.float64)
    assert (a >= 0).all() and (bb >= 0).all() and (a + bb <= 1 + 1e-15).all()
    got = X.uv(t, b)
    assert got.dtype == np.float32 and np.allclose(got * np.array([lay["W"], lay["H"]]), c, rtol=0, atol=1e-3)


def test_refusals_need_no_gpu():
    X.assert_refusals(hip)
    for bad in ((-1, 8), (4, 3), (4, 65), (2 * 4096 * 4096 + 1, 4)):
        with pytest.raises(hip.MnerfError):
            hip.mesh_texture_atlas(*bad)


def test_python_layers_refuse_before_any_launch():
    from matchnerf_amd.matchnerf import MatchNeRF
    for block, power in ((3, 2), (65, 2), (7.5, 2), (8, -1), (8, 9), (8, 1.5)):
        with pytest.raises(ValueError):
            fusion._texture_block("test", block, power)
        with pytest.raises(ValueError):
            MatchNeRF.check_texture("test", block, power, "render", "sources")
    assert fusion._texture_block("test", 0, 0) == (0, 0) and fusion._texture_block("test", 8.0, 2) == (8, 2)
    with pytest.raises(ValueError, match="images"):
        MatchNeRF.check_texture("test", 8, 2, "images", "path")
    with pytest.raises(ValueError, match="texture_from"):
        MatchNeRF.check_texture("test", 8, 2, "photos", "sources")
    assert MatchNeRF.check_texture("test", 8, 2, "images", "sources") == (8, 2)
    with pytest.raises(ValueError):  # refused before a tensor is touched
        fusion.texture(None, None, [None] * 3, None, None, None, (4, 4), True, block=2)
    with pytest.raises(ValueError):
        fusion.mesh([None] * 3, None, None, None, (4, 4), True, texture=3)


@pytest.mark.parametrize("case", X.CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_fp32_restatement_reaches_the_gate_and_few_texels_are_borderline(case):
    """the 1e-4 RGB gate of the GPU test is reachable in the device's format, and every case it uses leaves out at most the cap"""
    s = X.scene(*case)
    assert 500 < len(s["faces"]) < 10000
    for block in X.BLOCKS:
        width, height = X.atlas_size(len(s["faces"]), block)[:2]
        assert width < 512 and height < 512
        for best in (False, True):
            r = X.baked(*case, block, best)
            err, alpha, share = X.atlas_distance(r["atlas32"], r["atlas"], r["border"])
            seen = float(r["atlas"][..., 3].mean())
            print(f"texture {case} B={block} best={best}: atlas {width}x{height}, {len(s['faces'])} triangles, a=1 on {seen:.3f}, borderline "
                  f"{share:.5f}, fp32 vs fp64 rgb {err:.2e}, alpha differs on {alpha}")
            assert share <= X.BORDERLINE_CAP, (case, block, best, share)
            assert err <= X.RGB_GATE and alpha == 0, (case, block, best, err, alpha)
            assert seen > 0.2  # the cameras see a good part of the surface: the case tests the accumulation, not the fallback
            unowned = X.layout(len(s["faces"]), block)["owner"] < 0
            assert not r["atlas"][unowned].any()


def decimated_scene(case, cell_voxels=3):
    """the case's mesh decimated by the restatement with cells of ``cell_voxels`` voxels on the volume's grid"""
    s = X.scene(*case)
    dims = tuple(int(np.ceil(d / cell_voxels)) for d in s["dims"])
    d = D.decimate(s["vertices"], s["faces"], s["origin"], cell_voxels * s["voxel"], dims)
    return s, d["vertices"], d["faces"]


def test_purpose_the_atlas_is_closer_to_the_colour_field_than_the_vertex_colours():
    case = (16, 37, 53, False, "plain", False)
    s, vertices, faces = decimated_scene(case)
    assert 20 < len(faces) < len(s["faces"]) // 3
    acc, _ = X.accumulate(vertices, faces, 8, s["cams"], case[1], case[2], case[3], s["depth"], s["opacity"], s["rgb"])
    atlas = X.resolve(vertices, faces, 8, acc)
    textured, plain, seen = X.colour_errors(vertices, faces, 8, atlas, s["voxel"])
    print(f"purpose {case}, cells of 3 voxels, {len(faces)} triangles: RMS colour error {textured:.4f} with the atlas, {plain:.4f} with "
          f"the vertex colours, over the {seen:.3f} of the samples that a view saw")
    assert seen > 0.3 and textured < plain


def test_write_obj_round_trip(tmp_path):
    from PIL import Image
    vertices = np.array([[0, 0, 0, 1, .1, .2, .3, 0], [1, 0, 0, 1, .4, .5, .6, 0], [0, 1, 0.5, 1, .7, .8, .9, 0], [1, 1, 0.25, 1, 1, 0, 1, 0]], np.float32)
    faces = np.array([[0, 1, 2], [2, 1, 3]], np.int32)
    uv = X.uv(2, 4)
    width, height = X.atlas_size(2, 4)[:2]
    rng = np.random.default_rng(4)
    atlas = rng.uniform(-0.2, 1.2, (height, width, 4)).astype(np.float32)
    atlas[0, 0, :3] = (0.5, np.nan, 0.002)
    normals = rng.normal(size=(4, 4)).astype(np.float32)
    for nrm in (None, normals):
        path = tmp_path / ("with_normals.obj" if nrm is not None else "plain.obj")
        assert fusion.write_obj(str(path), vertices, faces, uv, atlas, nrm) == 4
        stem = path.stem
        lines = path.read_text().splitlines()
        kinds = [l.split()[0] for l in lines]
        assert lines[0] == f"mtllib {stem}.mtl" and lines[1] == f"usemtl {stem}"
        assert kinds.count("v") == 4 and kinds.count("vt") == 6 and kinds.count("vn") == (4 if nrm is not None else 0) and kinds.count("f") == 2
        assert len(lines) == 2 + 4 + 6 + 2 + (4 if nrm is not None else 0)
        got_v = np.array([[float(x) for x in l.split()[1:]] for l in lines if l.startswith("v ")], np.float32)
        assert np.array_equal(got_v, vertices[:, :3])
        got_vt = np.array([[float(x) for x in l.split()[1:]] for l in lines if l.startswith("vt ")])
        assert np.array_equal(got_vt[:, 0].astype(np.float32), uv.reshape(-1, 2)[:, 0])
        assert np.array_equal(got_vt[:, 1], 1.0 - uv.reshape(-1, 2)[:, 1].astype(np.float64))  # v flipped: OBJ's origin is bottom-left
        f = [l.split()[1:] for l in lines if l.startswith("f ")]
        if nrm is None:
            assert f == [["1/1", "2/2", "3/3"], ["3/4", "2/5", "4/6"]]
        else:
            assert f == [["1/1/1", "2/2/2", "3/3/3"], ["3/4/3", "2/5/2", "4/6/4"]]
            got_n = np.array([[float(x) for x in l.split()[1:]] for l in lines if l.startswith("vn ")], np.float32)
            assert np.array_equal(got_n, normals[:, :3])
        mtl = (tmp_path / f"{stem}.mtl").read_text()
        assert f"newmtl {stem}\n" in mtl and f"map_Kd {stem}.png\n" in mtl
        img = Image.open(tmp_path / f"{stem}.png")
        assert img.size == (width, height) and img.mode == "RGB"
        want = np.rint(np.clip(np.nan_to_num(atlas[..., :3].astype(np.float64)), 0.0, 1.0) * 255.0).astype(np.uint8)
        assert np.array_equal(np.asarray(img), want) and tuple(want[0, 0]) == (128, 0, 1)
    with pytest.raises(ValueError):
        fusion.write_obj(str(tmp_path / "bad.obj"), vertices, faces, uv[:1], atlas)
    with pytest.raises(ValueError):
        fusion.write_obj(str(tmp_path / "bad.obj"), vertices, faces + 2, uv, atlas)
