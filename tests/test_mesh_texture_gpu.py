"""Mesh texture on the GPU (include/mnerf.h "MESH TEXTURE", matchnerf_amd/csrc/mesh_texture.hip) against the numpy restatement of
tests/mesh_texture_helpers.py.

uv: bit for bit.  Accumulate + resolve: rgb within 1e-4 (the project's RGB gate) of the float64 restatement on the texels that are
not BORDERLINE (at most 1 % of a case, tests/test_mesh_texture_cpu.py), alpha equal there, texels without an owner exactly 0; the
fallback colours bit for bit the fp32 restatement's (two FMAs).  Every output lies between guard regions that must stay untouched,
and the inputs are compared bitwise afterwards."""
import numpy as np
import pytest
import torch

import fusion_helpers as F
import mesh_helpers as M
import mesh_texture_helpers as X
from test_mesh_finish_gpu import Guarded, _bits, _cuda

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from matchnerf_amd import hip as h
    h.load()
    assert torch.cuda.is_available(), "the gpu-marked tests need a GPU"
    return h


def _views(hip, cams):
    return [hip.make_view(c["extr"], c["intr"], c["near"], c["far"]) for c in cams]


class Inputs:
    """the device copies of a bake's inputs, and the check that no launch wrote them"""

    def __init__(self, hip, vertices, faces, cams, depth, opacity, rgb, counts=None):
        self.host = dict(vertices=np.ascontiguousarray(vertices, np.float32), faces=np.ascontiguousarray(faces, np.int32),
                         depth=np.ascontiguousarray(depth, np.float32), rgb=np.ascontiguousarray(rgb, np.float32))
        if opacity is not None:
            self.host["opacity"] = np.ascontiguousarray(opacity, np.float32)
        if counts is not None:
            self.host["counts"] = np.ascontiguousarray(counts, np.int32)
        self.dev = {k: _cuda(v) for k, v in self.host.items()}
        self.views = _views(hip, cams)

    def get(self, name):
        return self.dev.get(name)

    def unwritten(self):
        return all(np.array_equal(self.dev[k].cpu().numpy().view(np.uint32), v.view(np.uint32)) for k, v in self.host.items())


def _bake(hip, inp, block, legacy, min_consistent=0, best=False, in_place=False, groups=None, **kwargs):
    """guarded accum and atlas -> (atlas numpy [H, W, 4], accum numpy); ``groups``: the view ranges of the accumulate calls"""
    n_faces = inp.host["faces"].shape[0]
    width, height = hip.mesh_texture_atlas(n_faces, block)
    accum, atlas = Guarded(4 * width * height, torch.float32), Guarded(4 * width * height, torch.float32)
    accum.t.zero_()
    k = len(inp.views)
    for group in groups or [slice(0, k)]:
        hip.mesh_texture_accumulate(inp.get("vertices"), inp.get("faces"), block, inp.views[group], inp.get("depth")[group], inp.get("rgb")[group],
                                    accum.t.view(height, width, 4), opacity=None if inp.get("opacity") is None else inp.get("opacity")[group],
                                    n_consistent=None if inp.get("counts") is None else inp.get("counts")[group],
                                    min_consistent=min_consistent, legacy=legacy, best=best, **kwargs)
    summed = accum.t.cpu().numpy().reshape(height, width, 4)
    out = accum if in_place else atlas
    hip.mesh_texture_resolve(inp.get("vertices"), inp.get("faces"), block, accum.t.view(height, width, 4), best=best,
                             out=out.t.view(height, width, 4))
    torch.cuda.synchronize()
    assert accum.untouched() and atlas.untouched() and inp.unwritten()
    if not in_place:
        assert np.array_equal(_bits(accum.t.cpu().numpy().reshape(height, width, 4)), _bits(summed))  # resolve reads accum only
    return out.t.cpu().numpy().reshape(height, width, 4), summed


# ------------------------------------------------------------------------------------------------ uv
@pytest.mark.parametrize("t", X.LAYOUT_T)
def test_uv_is_the_restatement_bit_for_bit(hip, t):
    for b in X.LAYOUT_B:
        want = X.uv(t, b)
        out = Guarded(6 * t, torch.float32)
        got = hip.mesh_texture_uv(t, b, out=out.t)
        torch.cuda.synchronize()
        assert out.untouched() and got.shape == (t, 3, 2)
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)), (t, b)
        assert hip.mesh_texture_atlas(t, b) == X.atlas_size(t, b)[:2]
    assert hip.mesh_texture_uv(t, 8, device="cuda").shape == (t, 3, 2)


# ------------------------------------------------------------------------------------------------ accumulate + resolve
@pytest.mark.parametrize("case", X.CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_bake_against_float64(hip, case):
    k, h, w, legacy, variant, consistent = case
    s = X.scene(*case)
    inp = Inputs(hip, s["vertices"], s["faces"], s["cams"], s["depth"], s["opacity"], s["rgb"], s["counts"])
    for block in X.BLOCKS:
        unowned = X.layout(len(s["faces"]), block)["owner"] < 0
        for best in (False, True):
            want = X.baked(*case, block, best)
            got, _ = _bake(hip, inp, block, legacy, min_consistent=s["min_consistent"], best=best)
            err, alpha, share = X.atlas_distance(got, want["atlas"], want["border"])
            print(f"texture {case} B={block} best={best}: {got.shape[1]}x{got.shape[0]}, rgb within {err:.2e} of float64, alpha differs on "
                  f"{alpha}, borderline {share:.5f}; bits equal to the fp32 restatement on "
                  f"{float((_bits(got) == _bits(want['atlas32'])).all(-1).mean()):.4f} of the texels")
            assert share <= X.BORDERLINE_CAP
            assert err <= X.RGB_GATE and alpha == 0, (case, block, best, err, alpha)
            assert not _bits(got)[unowned].any()  # exactly 0, no -0.0
            assert float(got[..., 3].mean()) > 0.2


# ------------------------------------------------------------------------------------------------ hand-made meshes
HAND = (3, 24, 32, False, "plain")


def _hand(hip, kind, best=False, block=8):
    s = F.scene(*HAND)
    cams = s["cams"]
    rgb = X.view_colours(cams, 24, 32, False, s["depth"], None, 0.1)
    vertices, faces = X.hand_mesh(kind)
    inp = Inputs(hip, vertices, faces, cams, s["depth"], None, rgb)
    got, summed = _bake(hip, inp, block, False, best=best)
    args = (vertices, faces, block, cams, 24, 32, False, s["depth"], None, rgb)
    acc64, border = X.accumulate(*args, best=best)
    acc32, _ = X.accumulate(*args, best=best, dtype=np.float32)
    return dict(got=got, summed=summed, want=X.resolve(vertices, faces, block, acc64, best), border=border,
                want32=X.resolve(vertices, faces, block, acc32, best, np.float32), layout=X.layout(len(faces), block))


@pytest.mark.parametrize("best", [False, True])
def test_one_triangle_facing_the_cameras(hip, best):
    r = _hand(hip, "facing", best)
    got, owner = r["got"], r["layout"]["owner"]
    assert got.shape == (8, 8, 4) and (owner == 0).sum() == 36 and (owner == -1).sum() == 28  # T odd: the upper half has no owner
    assert not _bits(got)[owner < 0].any()
    assert (got[..., 3][owner == 0] == 1.0).all()  # every view sees the box's front face
    err, alpha, _ = X.atlas_distance(got, r["want"], r["border"])
    assert err <= X.RGB_GATE and alpha == 0
    assert got[..., :3][owner == 0].std() > 0.05  # the field's detail, not one colour


@pytest.mark.parametrize("kind", ["back", "occluded"])
def test_unseen_triangles_fall_back_to_the_vertex_colours(hip, kind):
    for best in (False, True):
        r = _hand(hip, kind, best)
        owner = r["layout"]["owner"]
        assert not r["summed"].any()  # no view contributed
        assert (r["got"][..., 3] == 0.0).all() and (r["want"][..., 3] == 0.0).all()
        assert np.array_equal(_bits(r["got"]), _bits(r["want32"]))  # the two FMAs, bit for bit
        assert r["got"][..., :3][owner == 0].std() > 0.01 and not _bits(r["got"])[owner < 0].any()


def test_broken_triangles_are_zero_and_leave_their_neighbours_alone(hip):
    r = _hand(hip, "broken")
    got, owner = r["got"], r["layout"]["owner"]
    for t in (1, 2, 3):  # degenerate, an index >= V, a NaN vertex
        assert (owner == t).sum() > 0 and not _bits(got)[owner == t].any() and not r["summed"][owner == t].any()
    for t in (0, 4):
        assert (got[..., 3][owner == t] == 1.0).all()
    assert np.isfinite(got).all()
    err, alpha, _ = X.atlas_distance(got, r["want"], r["border"])
    assert err <= X.RGB_GATE and alpha == 0
    # triangle 0 is the lone triangle of "facing": the broken neighbours change none of its texels
    alone = _hand(hip, "facing")
    assert np.array_equal(_bits(got[:8, :8][alone["layout"]["owner"] == 0]), _bits(alone["got"][alone["layout"]["owner"] == 0]))


# ------------------------------------------------------------------------------------------------ in place, determinism, groups
def test_in_place_resolve_and_two_runs_give_the_same_bytes(hip):
    case = (3, 24, 32, False, "opacity", False)
    s = X.scene(*case)
    inp = Inputs(hip, s["vertices"], s["faces"], s["cams"], s["depth"], s["opacity"], s["rgb"])
    for best in (False, True):
        first, _ = _bake(hip, inp, 5, False, best=best)
        again, _ = _bake(hip, inp, 5, False, best=best)
        in_place, _ = _bake(hip, inp, 5, False, best=best, in_place=True)
        assert np.array_equal(_bits(first), _bits(again)) and np.array_equal(_bits(first), _bits(in_place))


def test_seventeen_views_in_two_calls(hip):
    from matchnerf_amd import fusion
    k, h, w, legacy = 17, 24, 32, False
    mesh = X.scene(3, h, w, legacy, "plain", False)  # the same world, meshed from three of its views
    s = F.scene(k, h, w, legacy)
    rgb = X.view_colours(s["cams"], h, w, legacy, s["depth"], None, mesh["voxel"])
    inp = Inputs(hip, mesh["vertices"], mesh["faces"], s["cams"], s["depth"], None, rgb)
    args = (mesh["vertices"], mesh["faces"], 8, s["cams"][:16], h, w, legacy, s["depth"][:16], None, rgb[:16])
    rest = (mesh["vertices"], mesh["faces"], 8, s["cams"][16:], h, w, legacy, s["depth"][16:], None, rgb[16:])
    for best in (False, True):
        got, _ = _bake(hip, inp, 8, legacy, best=best, groups=[slice(0, 16), slice(16, 17)])
        uv, atlas = fusion.texture(inp.get("vertices"), inp.get("faces"), inp.views, inp.get("depth"), None, inp.get("rgb"), (h, w), legacy,
                                   block=8, consistency=False, best=best)
        assert np.array_equal(_bits(atlas.cpu().numpy()), _bits(got)) and np.array_equal(_bits(uv.cpu().numpy()), _bits(X.uv(len(mesh["faces"]), 8)))
        acc, border = X.accumulate(*args, best=best)
        acc, border2 = X.accumulate(*rest, best=best, accum=acc)  # the 17 views in order: one sum
        err, alpha, share = X.atlas_distance(got, X.resolve(mesh["vertices"], mesh["faces"], 8, acc, best), border | border2)
        acc32, _ = X.accumulate(*args, best=best, dtype=np.float32)
        acc32, _ = X.accumulate(*rest, best=best, dtype=np.float32, accum=acc32)
        want32 = X.resolve(mesh["vertices"], mesh["faces"], 8, acc32, best, np.float32)
        err32, alpha32, _ = X.atlas_distance(got, want32.astype(np.float64), border | border2)
        print(f"17 views, best={best}: rgb within {err:.2e} of the float64 sum and {err32:.2e} of the fp32 sum over all views in order, "
              f"borderline {share:.5f}")
        assert err <= X.RGB_GATE and alpha == 0
        if not best:
            assert err32 <= 1e-6 and alpha32 == 0


# ------------------------------------------------------------------------------------------------ the module's functions
def _same_bytes(a, b):
    return all(x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def test_fusion_mesh_textures_the_finished_mesh(hip):
    from matchnerf_amd import fusion
    k, h, w, legacy = 16, 37, 53, False
    s = F.scene(k, h, w, legacy)
    origin, voxel, dims, _ = M.grid_of(k)
    rgb = X.view_colours(s["cams"], h, w, legacy, s["depth"], None, voxel)
    views, depth, colours = _views(hip, s["cams"]), _cuda(s["depth"]), _cuda(rgb)
    grid = dict(bounds=(origin, tuple(origin[a] + dims[a] * voxel for a in range(3))), voxel=voxel)
    plain = fusion.mesh(views, depth, None, colours, (h, w), legacy, decimate=3, **grid)
    assert len(plain) == 2 and _same_bytes(plain, fusion.mesh(views, depth, None, colours, (h, w), legacy, decimate=3, texture=0, **grid))
    got = fusion.mesh(views, depth, None, colours, (h, w), legacy, decimate=3, texture=8, **grid)
    assert len(got) == 4 and _same_bytes(got[:2], plain)  # the mesh is what it is without the texture
    assert _same_bytes(got, fusion.mesh(views, depth, None, colours, (h, w), legacy, decimate=3, texture=8, **grid))
    vertices, faces, uv, atlas = got
    n_faces = faces.shape[0]
    width, height = hip.mesh_texture_atlas(n_faces, 8)
    assert n_faces > 20 and uv.shape == (n_faces, 3, 2) and atlas.shape == (height, width, 4)
    assert np.array_equal(_bits(uv.cpu().numpy()), _bits(X.uv(n_faces, 8)))
    # the same launches through fusion.texture: the consistency maps computed there are the ones fusion.mesh reused
    assert _same_bytes(fusion.texture(vertices, faces, views, depth, None, colours, (h, w), legacy, block=8), (uv, atlas))
    textured, vertex, seen = X.colour_errors(vertices.cpu().numpy(), faces.cpu().numpy(), 8, atlas.cpu().numpy(), voxel)
    print(f"fusion.mesh texture=8 decimate=3: {n_faces} triangles, atlas {width}x{height}, RMS colour error {textured:.4f} with the atlas, "
          f"{vertex:.4f} with the vertex colours, over the {seen:.3f} of the samples that a view saw")
    assert seen > 0.3 and textured < vertex
    # other colours for the atlas leave the mesh alone
    other = fusion.mesh(views, depth, None, colours, (h, w), legacy, decimate=3, texture=8, texture_rgbs=1.0 - colours, **grid)
    assert _same_bytes(other[:3], got[:3]) and not torch.equal(other[3], atlas)
    for bad in (dict(texture=3), dict(texture=65), dict(texture=8, texture_power=9), dict(texture=7.5)):
        with pytest.raises(ValueError):
            fusion.mesh(views, depth, None, colours, (h, w), legacy, **bad, **grid)


def test_argument_refusals_precede_any_launch(hip):
    X.assert_refusals(hip)
    s = X.scene(3, 24, 32, False, "plain", False)
    inp = Inputs(hip, s["vertices"], s["faces"], s["cams"], s["depth"], None, s["rgb"])
    v, f, d, c = inp.get("vertices"), inp.get("faces"), inp.get("depth"), inp.get("rgb")
    width, height = hip.mesh_texture_atlas(f.shape[0], 8)
    guard = Guarded(4 * width * height, torch.float32)
    accum = guard.t.view(height, width, 4)
    acc = lambda *a, **k: hip.mesh_texture_accumulate(*a, **k)
    nan = float("nan")
    wrong = [lambda: acc(v, f, 3, inp.views, d, c, accum), lambda: acc(v, f, 65, inp.views, d, c, accum), lambda: acc(v, f, 5, inp.views, d, c, accum),
             lambda: acc(v, f.long(), 8, inp.views, d, c, accum), lambda: acc(v.cpu(), f, 8, inp.views, d, c, accum),
             lambda: acc(v, f, 8, inp.views[:2], d, c, accum), lambda: acc(v, f, 8, inp.views, d[:, :-1], c, accum),
             lambda: acc(v, f, 8, inp.views, d, c[:, :-1], accum), lambda: acc(v, f, 8, inp.views, d, c, accum, opacity=d[:2]),
             lambda: acc(v, f, 8, inp.views, d, c, accum, n_consistent=d), lambda: acc(v, f, 8, inp.views, d, c, accum, power=9),
             lambda: acc(v, f, 8, inp.views, d, c, accum, power=1.5), lambda: acc(v, f, 8, inp.views, d, c, accum, vis_rel_tol=0.0),
             lambda: acc(v, f, 8, inp.views, d, c, accum, vis_rel_tol=nan), lambda: acc(v, f, 8, inp.views, d, c, accum.view(-1)[:-4]),
             lambda: acc(v, f, 8, inp.views, d, c, accum.double()),
             lambda: hip.mesh_texture_resolve(v, f, 8, accum.view(-1)[:-4]), lambda: hip.mesh_texture_resolve(v, f, 4, accum),
             lambda: hip.mesh_texture_resolve(v, f, 8, accum, out=accum.view(-1)[4:]), lambda: hip.mesh_texture_resolve(v, f, 3, accum),
             lambda: hip.mesh_texture_uv(f.shape[0], 3, device="cuda"), lambda: hip.mesh_texture_uv(-1, 8, device="cuda"),
             lambda: hip.mesh_texture_uv(f.shape[0], 8, out=torch.empty(6 * f.shape[0] - 1, device="cuda")),
             lambda: hip.mesh_texture_uv(f.shape[0], 8, out=torch.empty(6 * f.shape[0]))]
    for call in wrong:
        with pytest.raises(hip.MnerfError):
            call()
    torch.cuda.synchronize()
    assert guard.untouched() and bool((guard.t == guard.value).all()) and inp.unwritten()  # nothing was written
    guard.t.zero_()
    acc(v, f, 8, inp.views, d, c, accum)  # the same call without a flaw writes
    torch.cuda.synchronize()
    assert bool((accum[..., 3] > 0).any()) and guard.untouched()


def test_export_mesh_takes_the_texture_and_refuses_before_any_launch(hip):
    from test_fusion_gpu import LOOSE, _model
    opt, model, batch, calls = _model("nonlegacy")
    with torch.no_grad():
        for bad in (dict(texture=3), dict(texture=65), dict(texture=8, texture_power=9), dict(texture=8, texture_power=-1),
                    dict(texture=8, texture_from="photos"), dict(texture=8, texture_from="images", views="path")):
            with pytest.raises(ValueError):
                model.export_mesh(batch, **{**dict(views="sources", resolution=48), **bad}, **LOOSE)
        assert len(calls) == 0  # refused before the encoder ran
        plain = model.export_mesh(batch, views="sources", resolution=48, decimate=3, **LOOSE)
        render = model.export_mesh(batch, views="sources", resolution=48, decimate=3, texture=8, normals=True, **LOOSE)
        images = model.export_mesh(batch, views="sources", resolution=48, decimate=3, texture=8, texture_from="images", texture_best=True,
                                   **LOOSE)
    vertices, faces, normals, uv, atlas = render[0]
    assert _same_bytes((vertices, faces), plain[0]) and _same_bytes(images[0][:3], (vertices, faces, uv))
    width, height = hip.mesh_texture_atlas(faces.shape[0], 8)
    assert normals.shape == (vertices.shape[0], 4) and uv.shape == (faces.shape[0], 3, 2) and atlas.shape == (height, width, 4)
    for a in (atlas, images[0][3]):
        assert bool(torch.isfinite(a).all()) and float(a[..., 3].mean()) > 0.05 and set(a[..., 3].unique().tolist()) <= {0.0, 1.0}
    assert not torch.equal(images[0][3], atlas)


def test_coach_export_geometry_writes_the_textured_mesh(hip, tmp_path, monkeypatch):
    from PIL import Image
    from test_fusion_gpu import _coach
    loose = ["--nerf.export_geometry=sources", "--nerf.fuse_px_tol=64", "--nerf.fuse_rel_tol=0.9", "--nerf.fuse_min_opacity=0.01",
             "--nerf.fuse_min_views=1", "--nerf.export_mesh", "--nerf.mesh_resolution=48", "--nerf.mesh_normals", "--nerf.mesh_decimate=3"]
    c = _coach(tmp_path, monkeypatch, *loose)
    written = c.export_geometry()["dtu"]
    assert len(written) == 2
    before = open(written[1], "rb").read()
    c.opts.nerf.mesh_texture = 8
    written = c.export_geometry()["dtu"]
    assert len(written) == 3 and written[1].endswith("_mesh.ply") and written[2].endswith("_mesh.obj")
    assert open(written[1], "rb").read() == before  # the PLY is the bytes it was
    stem = written[2][:-len(".obj")]
    lines = open(written[2]).read().splitlines()
    kinds = [l.split()[0] for l in lines]
    n_faces = kinds.count("f")
    assert n_faces > 0 and kinds.count("vt") == 3 * n_faces and kinds.count("vn") == kinds.count("v") > 0
    assert "map_Kd " + stem.split("/")[-1] + ".png" in open(stem + ".mtl").read()
    with Image.open(stem + ".png") as im:
        assert im.mode == "RGB" and im.size == hip.mesh_texture_atlas(n_faces, 8) and np.asarray(im).std() > 0
    first = {ext: open(stem + ext, "rb").read() for ext in (".obj", ".mtl", ".png")}
    c.opts.nerf.mesh_texture_from = "images"
    c.opts.nerf.mesh_texture_best = True
    c.export_geometry()
    assert open(stem + ".obj", "rb").read() == first[".obj"] and open(stem + ".png", "rb").read() != first[".png"]
    c.opts.nerf.mesh_texture = 3
    with pytest.raises(ValueError, match="mesh_texture"):
        c.export_geometry()
