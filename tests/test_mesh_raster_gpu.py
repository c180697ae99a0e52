"""Mesh raster on the GPU (include/mnerf.h "MESH RASTER", matchnerf_amd/csrc/mesh_raster.hip) against the numpy restatement of
tests/mesh_raster_helpers.py.

Hand-made meshes on integer pixels: exact.  The project's analytic meshes: on the pixels that are not BORDERLINE (at most 1 % of a
case, tests/test_mesh_raster_cpu.py) the face and hit / no-hit of the float64 restatement, depth and weights within 4 x the float32
restatement's own distance from float64, colours within 1e-4 - and every output bit for bit the float32 restatement's.  Every output lies between guard regions that must stay untouched, and
the inputs are compared bitwise afterwards."""
import json

import numpy as np
import pytest
import torch

import fusion_helpers as F
import mesh_raster_helpers as R
import mesh_texture_helpers as X
from test_mesh_finish_gpu import Guarded, _bits, _cuda

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from matchnerf_amd import hip as h
    h.load()
    assert torch.cuda.is_available(), "the gpu-marked tests need a GPU"
    return h


def _view(hip, c, near=None, far=None):
    return hip.make_view(c["extr"], c["intr"], c["near"] if near is None else near, c["far"] if far is None else far)


class Mesh:
    """the device copies of a mesh (and an atlas), and the check that no launch wrote them"""

    def __init__(self, vertices, faces, atlas=None):
        self.host = dict(vertices=np.ascontiguousarray(vertices, np.float32).reshape(-1, 8), faces=np.ascontiguousarray(faces, np.int32).reshape(-1, 3))
        if atlas is not None:
            self.host["atlas"] = np.ascontiguousarray(atlas, np.float32)
        self.dev = {k: _cuda(v) for k, v in self.host.items()}
        if len(self.host["vertices"]) == 0:
            self.dev["vertices"] = torch.empty(0, 8, device="cuda")
        if len(self.host["faces"]) == 0:
            self.dev["faces"] = torch.empty(0, 3, dtype=torch.int32, device="cuda")

    def unwritten(self):
        return all(np.array_equal(self.dev[k].cpu().numpy().view(np.uint32), v.view(np.uint32)) for k, v in self.host.items())


def _frame(hip, mesh, view, h, w, legacy, block=0, normals=False, fill=None, workspace=None):
    """guarded outputs of one raster and its shadings -> dict of numpy arrays (rgba: vertex colours; tex: from the atlas)"""
    outs = dict(face=Guarded(h * w, torch.int32), depth=Guarded(h * w, torch.float32), bary=Guarded(2 * h * w, torch.float32),
                rgba=Guarded(4 * h * w, torch.float32), tex=Guarded(4 * h * w, torch.float32), normal=Guarded(4 * h * w, torch.float32))
    if fill is not None:
        for g in outs.values():
            g.t.fill_(fill)
    v, f = mesh.dev["vertices"], mesh.dev["faces"]
    face, depth, bary = hip.mesh_raster(v, f, view, (h, w), legacy=legacy, out=(outs["face"].t, outs["depth"].t, outs["bary"].t), workspace=workspace)
    got = hip.mesh_shade(v, f, face, bary, view, normals=normals, out=(outs["rgba"].t, outs["normal"].t) if normals else outs["rgba"].t)
    if "atlas" in mesh.dev:
        hip.mesh_shade(v, f, face, bary, view, atlas=mesh.dev["atlas"], block=block, out=outs["tex"].t)
    torch.cuda.synchronize()
    assert all(g.untouched() for g in outs.values()) and mesh.unwritten()
    assert face.shape == (h, w) and depth.shape == (h, w) and bary.shape == (h, w, 2)
    assert (got[0] if normals else got).shape == (h, w, 4)
    shape = dict(face=(h, w), depth=(h, w), bary=(h, w, 2), rgba=(h, w, 4), tex=(h, w, 4), normal=(h, w, 4))
    return {k: g.t.cpu().numpy().reshape(shape[k]) for k, g in outs.items()}


def _consistent(got):
    """what holds for every frame: no hit <=> face == -1 <=> depth, weights and colour are exactly 0"""
    miss = got["face"] < 0
    assert (got["face"][miss] == -1).all() and np.array_equal(_bits(got["depth"]) == 0, miss)
    assert not _bits(got["bary"])[miss].any() and not _bits(got["rgba"])[miss].any()
    assert (got["rgba"][..., 3][~miss] == 1.0).all() and (got["depth"][~miss] > 0).all()


# ------------------------------------------------------------------------------------------------ 1. hand-made meshes, exact
HAND_FRAMES = ((24, 32), (37, 53), (1, 1))


def _hand(hip, vertices, faces, h, w):
    cam = R.pixel_camera()
    got = _frame(hip, Mesh(vertices, faces), _view(hip, cam), h, w, True)
    _consistent(got)
    want = R.raster(vertices, faces, cam, h, w, True)
    want32 = R.raster(vertices, faces, cam, h, w, True, np.float32)
    assert np.array_equal(got["face"], want["face"]) and np.array_equal(want32["face"], want["face"])
    assert np.array_equal(_bits(got["depth"]), _bits(want32["depth"])) and np.array_equal(_bits(got["bary"]), _bits(want32["bary"]))
    rgba, _ = R.shade(vertices, faces, want32["face"], want32["bary"], cam, dtype=np.float32)
    assert np.array_equal(_bits(got["rgba"]), _bits(rgba))
    return got


@pytest.mark.parametrize("hw", HAND_FRAMES)
def test_hand_meshes_are_exact(hip, hw):
    h, w = hw
    for kind in ("quad", "quad_unwelded"):
        got = _hand(hip, *R.hand_mesh(kind), h, w)
        want = R.top_left_set(0, 0, 8, 8, h, w)
        assert np.array_equal(got["face"] >= 0, want) and (got["face"] >= 0).sum() == min(h, 8) * min(w, 8)  # 64: no hole on the diagonal
        assert (got["depth"][want] == 2.0).all()
    got = _hand(hip, *R.hand_mesh("fan"), h, w)
    if h > 9:
        assert got["face"][9, 10] >= 0 and set(np.unique(got["face"])) == {-1, 0, 1, 2, 3, 4, 5}
    got = _hand(hip, *R.hand_mesh("coincident"), h, w)
    assert set(np.unique(got["face"])) <= {-1, 0} and ((got["face"] == 0).any() or h < 9)  # the lower index wins
    got = _hand(hip, *R.hand_mesh("huge"), h, w)
    assert (got["face"] == 0).all()  # larger than the frame
    got = _hand(hip, *R.hand_mesh("nothing"), h, w)
    assert (got["face"] == -1).all()  # outside, behind, across the camera plane, without area
    vertices, faces = R.hand_mesh("broken")
    got = _hand(hip, vertices, faces, h, w)
    assert set(np.unique(got["face"])) <= {-1, 0, 4} and np.isfinite(got["rgba"]).all()
    for t in (0, 4):  # the neighbours of the skipped triangles are what they are alone
        alone = _hand(hip, vertices, faces[[t]], h, w)
        assert np.array_equal(got["face"] == t, alone["face"] == 0)
        assert np.array_equal(_bits(got["depth"])[got["face"] == t], _bits(alone["depth"])[alone["face"] == 0])


@pytest.mark.parametrize("t", [0, 1, 3, 4, 5])
def test_triangle_counts_around_the_workgroup(hip, t):
    """four triangles per workgroup: the tail, and T = 0 (the empty frame; nothing but clear and resolve is launched)"""
    pixels = [p for k in range(t) for p in ((1 + 6 * k, 1), (6 + 6 * k, 2), (2 + 6 * k, 9))]
    vertices = R.rows(pixels, z=[2.0 + (k // 3) for k in range(3 * t)]) if t else np.zeros((0, 8), np.float32)
    faces = np.arange(3 * t, dtype=np.int32).reshape(t, 3)
    got = _hand(hip, vertices, faces, 24, 32)
    assert set(np.unique(got["face"])) == set(range(-1, t))


# ------------------------------------------------------------------------------------------------ 2. the analytic meshes
BIT_DIFFERENCES = {}


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_analytic_meshes_against_float64(hip, case):
    name, decimated, k, h, w, legacy = case
    m, frames = R.mesh_of(*case), R.rastered(*case)
    atlas, block = R.atlas_of(*case)
    mesh = Mesh(m["vertices"], m["faces"], atlas)
    workspace = torch.empty(hip.mesh_raster_workspace_bytes(h, w), dtype=torch.uint8, device="cuda")  # one for all views
    worst = dict(depth=0.0, bary=0.0, rgb=0.0, tex=0.0)
    bits = dict(face=0, depth=0, bary=0, rgba=0, tex=0)
    share = 0.0
    for cam, want in zip(m["cams"], frames):
        got = _frame(hip, mesh, _view(hip, cam), h, w, legacy, block=block, normals=True, workspace=workspace)
        _consistent(got)
        keep = ~want["border"]
        share += float(want["border"].mean()) / k
        assert np.array_equal(got["face"][keep], want["face"][keep])  # the winner, and with it hit / no-hit
        d, b = R.frame_distance(got["depth"], got["bary"], want, keep)
        worst["depth"], worst["bary"] = max(worst["depth"], d), max(worst["bary"], b)
        on = keep & (want["face"] >= 0)
        rgba, normal = R.shade(m["vertices"], m["faces"], want["face"], want["bary"], cam)
        tex, _ = R.shade(m["vertices"], m["faces"], want["face"], want["bary"], cam, atlas, block)
        worst["rgb"] = max(worst["rgb"], float(np.abs(got["rgba"] - rgba)[on].max()))
        worst["tex"] = max(worst["tex"], float(np.abs(got["tex"] - tex)[on].max()))
        assert np.abs(got["normal"] - normal)[on].max() < 1e-4 and not _bits(got["normal"])[got["face"] < 0].any()
        rgba32, _ = R.shade(m["vertices"], m["faces"], want["face32"], want["bary32"], cam, dtype=np.float32)
        tex32, _ = R.shade(m["vertices"], m["faces"], want["face32"], want["bary32"], cam, atlas, block, np.float32)
        for key, ref in (("face", want["face32"]), ("depth", want["depth32"]), ("bary", want["bary32"]), ("rgba", rgba32), ("tex", tex32)):
            differs = _bits(got[key]) != _bits(np.ascontiguousarray(ref, got[key].dtype))
            bits[key] += int((differs.reshape(h, w, -1).any(-1) & keep).sum())
    BIT_DIFFERENCES[case] = bits
    print(f"raster {case}: {len(m['faces'])} triangles, borderline {share:.5f}; depth within {worst['depth']:.2e} (gate {R.DEPTH_GATE:.1e}), "
          f"weights {worst['bary']:.2e} (gate {R.BARY_GATE:.1e}), vertex colours {worst['rgb']:.2e}, atlas colours {worst['tex']:.2e} of "
          f"float64; pixels off the borderline whose bits differ from the float32 restatement: {bits}")
    assert share <= R.BORDERLINE_CAP
    assert worst["depth"] <= R.DEPTH_GATE and worst["bary"] <= R.BARY_GATE
    assert worst["rgb"] <= R.RGB_GATE and worst["tex"] <= R.RGB_GATE
    assert not any(bits.values())  # as the texture: the device IS the float32 restatement, bit for bit


# ------------------------------------------------------------------------------------------------ 3. watertightness
def test_the_closed_sphere_has_no_pinholes(hip):
    k, h, w = 16, 37, 53
    for legacy in (True, False):
        m = R.mesh_of("sphere", False, k, h, w, legacy)
        mesh = Mesh(m["vertices"], m["faces"])
        for cam in m["cams"]:
            got = _frame(hip, mesh, _view(hip, cam), h, w, legacy)
            inside = R.sphere_hits(cam, h, w, legacy, m["voxel"])
            assert inside.sum() > 0.2 * h * w and (got["face"][inside] >= 0).all()


# ------------------------------------------------------------------------------------------------ 4. determinism
def test_two_runs_into_other_buffers_give_the_same_bytes(hip):
    case = ("scene", False, 3, 24, 32, False)
    m = R.mesh_of(*case)
    atlas, block = R.atlas_of(*case)
    mesh = Mesh(m["vertices"], m["faces"], atlas)
    for cam in m["cams"]:
        view = _view(hip, cam)
        first = _frame(hip, mesh, view, 24, 32, False, block=block, normals=True, fill=0)
        again = _frame(hip, mesh, view, 24, 32, False, block=block, normals=True, fill=12345)
        for key in first:
            assert np.array_equal(_bits(first[key]), _bits(again[key])), key
        _consistent(first)


# ------------------------------------------------------------------------------------------------ 5. atlas isolation
def test_atlas_shading_reads_only_the_visible_triangles_texels(hip):
    for case in (("scene", False, 3, 24, 32, False), ("scene", True, 16, 37, 53, True)):
        name, decimated, k, h, w, legacy = case
        m = R.mesh_of(*case)
        atlas, block = R.atlas_of(*case)
        owner = X.layout(len(m["faces"]), block)["owner"]
        mesh = Mesh(m["vertices"], m["faces"], atlas)
        for cam in m["cams"][:4]:
            want = _frame(hip, mesh, _view(hip, cam), h, w, legacy, block=block)
            visible = np.unique(want["face"][want["face"] >= 0])
            poisoned = np.where(np.isin(owner, visible)[..., None], atlas, np.float32(np.nan))
            assert np.isnan(poisoned).any()
            got = _frame(hip, Mesh(m["vertices"], m["faces"], poisoned), _view(hip, cam), h, w, legacy, block=block)
            assert np.isfinite(got["tex"]).all() and np.array_equal(_bits(got["tex"]), _bits(want["tex"]))


# ------------------------------------------------------------------------------------------------ 6. visibility="mesh"
def test_texture_visibility_against_the_mesh(hip):
    """The decimated plane + box case with cells of 3 voxels, the smallest the issue names, shows the purpose: tested against the
    mesh's own depth more owned texels find a view (float64 restatements: 0.8897 against 0.8196 with the views' depth)."""
    from matchnerf_amd import fusion
    r = R.visibility_shares()
    s = r["scene"]
    k, h, w, legacy = R.VISIBILITY_CASE
    views = [_view(hip, c) for c in s["cams"]]
    v, f, depth, rgb = _cuda(r["vertices"]), _cuda(r["faces"]), _cuda(s["depth"]), _cuda(s["rgb"])
    block = R.SCENE_BLOCK
    owned = X.layout(len(r["faces"]), block)["owner"] >= 0
    same = lambda a, b: all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
    for consistency in (True, False):
        plain = fusion.texture(v, f, views, depth, None, rgb, (h, w), legacy, block=block, consistency=consistency)
        named = fusion.texture(v, f, views, depth, None, rgb, (h, w), legacy, block=block, consistency=consistency, visibility="views")
        assert same(plain, named)  # today's path, the same bytes
    by_mesh = fusion.texture(v, f, views, depth, None, rgb, (h, w), legacy, block=block, consistency=False, visibility="mesh")
    assert same(by_mesh, fusion.texture(v, f, views, depth, None, rgb, (h, w), legacy, block=block, visibility="mesh"))
    shares = {}
    for mode, (uv, atlas) in (("views", plain), ("mesh", by_mesh)):
        a = atlas.cpu().numpy()
        shares[mode] = float(a[..., 3][owned].mean())
        rms = X.colour_errors(r["vertices"], r["faces"], block, a, s["voxel"])[0]
        print(f"visibility={mode}: a = 1 on {shares[mode]:.4f} of the owned texels (float64 restatement {r[mode][0]:.4f}), colour RMS {rms:.4f} "
              f"(restatement {r[mode][1]:.4f})")
        assert abs(shares[mode] - r[mode][0]) <= 0.01
    assert shares["mesh"] > shares["views"]
    # the depth maps handed over are the raster's, with the rim of one pixel
    mesh_views, maps = fusion.mesh_depths(v, f, views, (h, w), legacy)
    want = R.dilate(np.stack([R.raster(r["vertices"], r["faces"], dict(c, near=0.0, far=3.0e38), h, w, legacy, np.float32)["depth"]
                              for c in s["cams"]]))
    assert float((_bits(maps.cpu().numpy()) != _bits(want)).mean()) <= R.BORDERLINE_CAP and mesh_views[0].far_ > 1e38
    with pytest.raises(ValueError):
        fusion.texture(v, f, views, depth, None, rgb, (h, w), legacy, block=block, visibility="field")
    through = fusion.mesh(views, depth, None, rgb, (h, w), legacy, decimate=3, texture=block, texture_visibility="mesh",
                          bounds=(s["origin"], tuple(s["origin"][a] + s["dims"][a] * s["voxel"] for a in range(3))), voxel=s["voxel"])
    default = fusion.mesh(views, depth, None, rgb, (h, w), legacy, decimate=3, texture=block,
                          bounds=(s["origin"], tuple(s["origin"][a] + s["dims"][a] * s["voxel"] for a in range(3))), voxel=s["voxel"])
    assert same(through[:3], default[:3]) and not torch.equal(through[3], default[3])
    assert same(through[2:], fusion.texture(*through[:2], views, depth, None, rgb, (h, w), legacy, block=block, visibility="mesh"))


# ------------------------------------------------------------------------------------------------ 7. report, end to end
def test_mesh_report_against_the_restatement(hip):
    from matchnerf_amd import fusion
    k, h, w, legacy = 3, 24, 32, False
    s = X.scene(k, h, w, legacy, "plain", False)
    views = [_view(hip, c) for c in s["cams"]]
    v, f = _cuda(s["vertices"]), _cuda(s["faces"])
    report = fusion.mesh_report(v, f, views, _cuda(s["depth"]), None, _cuda(s["rgb"]), (h, w), legacy)
    assert set(report) == {"views", "pooled"} and len(report["views"]) == k
    frames = [R.raster(s["vertices"], s["faces"], dict(c, near=0.0, far=3.0e38), h, w, legacy) for c in s["cams"]]
    z_field = s["depth"].astype(np.float64)
    field = np.isfinite(z_field) & (z_field > 0)
    rows = []
    for j, r in enumerate(frames + [None]):
        if r is None:  # pooled
            on, zm, fld, zf = (np.stack([q["face"] >= 0 for q in frames]), np.stack([q["depth"] for q in frames]), field, z_field)
            colour = np.stack([R.shade(s["vertices"], s["faces"], q["face"], q["bary"], c)[0][..., :3] for q, c in zip(frames, s["cams"])])
            truth = s["rgb"].reshape(k, h, w, 3)
        else:
            on, zm, fld, zf = r["face"] >= 0, r["depth"], field[j], z_field[j]
            colour = R.shade(s["vertices"], s["faces"], r["face"], r["bary"], s["cams"][j])[0][..., :3]
            truth = s["rgb"][j].reshape(h, w, 3)
        common = on & fld
        rel = np.abs(zm - zf)[common] / zf[common]
        mse = ((colour - truth)[common] ** 2).mean()
        rows.append(dict(coverage=common.sum() / fld.sum(), spurious=(on.sum() - common.sum()) / on.sum(), depth_rel_mean=rel.mean(),
                         depth_rel_median=np.median(rel), psnr=-10 * np.log10(mse), field_pixels=fld.sum(), mesh_pixels=on.sum(),
                         common_pixels=common.sum()))
    border = float(np.mean([r["border"].mean() for r in frames]))
    for got, want in zip(report["views"] + [report["pooled"]], rows):
        assert set(got) == set(fusion.REPORT_KEYS)
        print("mesh_report:", {key: round(float(x), 5) for key, x in got.items()})
        assert abs(got["coverage"] - want["coverage"]) <= 0.01 + border and abs(got["spurious"] - want["spurious"]) <= 0.01 + border
        assert abs(got["depth_rel_mean"] - want["depth_rel_mean"]) <= 1e-4 and abs(got["psnr"] - want["psnr"]) <= 0.1
        assert abs(got["depth_rel_median"] - want["depth_rel_median"]) <= 1e-3  # (torch takes the lower of two middle values)
        assert abs(got["common_pixels"] - want["common_pixels"]) <= 0.01 * h * w * (k if got is report["pooled"] else 1)
    assert 0.3 < report["pooled"]["coverage"] < 1.0 and report["pooled"]["depth_rel_mean"] < 0.05  # the mesh lies on the field's surface


def test_export_mesh_reports_and_refuses_before_any_launch(hip):
    from matchnerf_amd import fusion
    from test_fusion_gpu import LOOSE, _model
    opt, model, batch, calls = _model("nonlegacy")
    with torch.no_grad():
        for bad in (dict(texture=8, texture_visibility="field"), dict(texture_visibility=None)):
            with pytest.raises(ValueError):
                model.export_mesh(batch, views="sources", resolution=48, report=True, **bad, **LOOSE)
        assert len(calls) == 0  # refused before the encoder ran
        plain = model.export_mesh(batch, views="sources", resolution=48, decimate=3, **LOOSE)
        meshes, reports = model.export_mesh(batch, views="sources", resolution=48, decimate=3, report=True, **LOOSE)
        textured, reports_t = model.export_mesh(batch, views="sources", resolution=48, decimate=3, texture=8, texture_visibility="mesh",
                                                report=True, normals=True, **LOOSE)
    same = lambda a, b: all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
    assert same(meshes[0], plain[0]) and same(textured[0][:2], plain[0]) and len(textured[0]) == 5
    for report in (reports[0], reports_t[0]):
        assert set(report) == {"views", "pooled"} and len(report["views"]) == model.n_src_views
        assert all(set(row) == set(fusion.REPORT_KEYS) for row in report["views"] + [report["pooled"]])
        assert report["pooled"]["mesh_pixels"] > 0 and 0.0 <= report["pooled"]["coverage"] <= 1.0
    json.dumps(reports[0])  # plain numbers


def test_coach_export_geometry_writes_the_report_and_the_previews(hip, tmp_path, monkeypatch):
    from PIL import Image
    from test_fusion_gpu import _coach
    loose = ["--nerf.export_geometry=sources", "--nerf.fuse_px_tol=64", "--nerf.fuse_rel_tol=0.9", "--nerf.fuse_min_opacity=0.01",
             "--nerf.fuse_min_views=1", "--nerf.export_mesh", "--nerf.mesh_resolution=48", "--nerf.mesh_decimate=3", "--nerf.mesh_texture=8"]
    c = _coach(tmp_path, monkeypatch, *loose)
    out_dir = tmp_path / "outputs" / "geometry" / "geometry" / "dtu"
    listing = lambda: {p.name: p.read_bytes() for p in sorted(out_dir.iterdir())}
    written = c.export_geometry()["dtu"]
    absent = listing()  # the keywords absent
    assert len(written) == 3 and not any("report" in n or "preview" in n for n in absent)
    for p in out_dir.iterdir():
        p.unlink()
    c.opts.nerf.mesh_report, c.opts.nerf.mesh_preview, c.opts.nerf.mesh_texture_visibility = False, False, "views"
    assert c.export_geometry()["dtu"] == written and listing() == absent  # switched off: the same directory, byte for byte
    c.opts.nerf.mesh_report, c.opts.nerf.mesh_preview = True, True
    written = c.export_geometry()["dtu"]
    now = listing()
    assert all(now[n] == absent[n] for n in absent)  # what was written before is what it was
    stem = written[1][:-len("_mesh.ply")]
    with open(stem + "_mesh_report.json") as fh:
        report = json.load(fh)
    k = c.model.n_src_views
    assert set(report) == {"views", "pooled"} and len(report["views"]) == k
    assert set(report["pooled"]) == {"coverage", "spurious", "depth_rel_mean", "depth_rel_median", "psnr", "field_pixels", "mesh_pixels",
                                     "common_pixels"}
    previews = sorted(n for n in now if "_mesh_preview_" in n)
    assert len(previews) == k and len(written) == 3 + 1 + k
    for n in previews:
        with Image.open(out_dir / n) as im:
            assert im.size == (2 * 48, 32) and im.mode == "RGB" and np.asarray(im).std() > 0
    c.opts.nerf.mesh_texture_visibility = "mesh"
    c.export_geometry()
    assert listing()[stem.split("/")[-1] + "_mesh.ply"] == absent[stem.split("/")[-1] + "_mesh.ply"]
    c.opts.nerf.mesh_texture_visibility = "field"
    with pytest.raises(ValueError, match="mesh_texture_visibility"):
        c.export_geometry()


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_argument_refusals_precede_any_launch(hip):
    R.assert_refusals(hip)
    case = ("scene", True, 3, 24, 32, False)
    m = R.mesh_of(*case)
    atlas, block = R.atlas_of(*case)
    mesh = Mesh(m["vertices"], m["faces"], atlas)
    v, f, a = mesh.dev["vertices"], mesh.dev["faces"], mesh.dev["atlas"]
    view = _view(hip, m["cams"][0])
    h, w = 24, 32
    guards = dict(face=Guarded(h * w, torch.int32), depth=Guarded(h * w, torch.float32), bary=Guarded(2 * h * w, torch.float32),
                  rgba=Guarded(4 * h * w, torch.float32))
    out = (guards["face"].t, guards["depth"].t, guards["bary"].t)
    face, bary = guards["face"].t.view(h, w), guards["bary"].t
    small = torch.empty(8 * h * w - 8, dtype=torch.uint8, device="cuda")
    wrong = [lambda: hip.mesh_raster(v, f, view, (0, w), out=out), lambda: hip.mesh_raster(v, f, view, (65536, 32768)),
             lambda: hip.mesh_raster(v, f.long(), view, (h, w), out=out), lambda: hip.mesh_raster(v.cpu(), f, view, (h, w), out=out),
             lambda: hip.mesh_raster(v, f, view, (h, w), out=(out[0][:-1], out[1], out[2])),
             lambda: hip.mesh_raster(v, f, view, (h, w), out=(out[0], out[1].double(), out[2])),
             lambda: hip.mesh_raster(v, f, view, (h, w), out=(out[0], out[1], out[2][:-2])),
             lambda: hip.mesh_raster(v, f, view, (h, w), out=out, workspace=small),
             lambda: hip.mesh_raster(v, f, hip.make_view(m["cams"][0]["extr"], np.zeros((3, 3)), 0.5, 6.0), (h, w), out=out),
             lambda: hip.mesh_shade(v, f, face, bary, view, atlas=a, block=4, out=guards["rgba"].t),
             lambda: hip.mesh_shade(v, f, face, bary, view, atlas=a, block=65, out=guards["rgba"].t),
             lambda: hip.mesh_shade(v, f, face, bary, view, atlas=a.view(-1)[:-4], block=block, out=guards["rgba"].t),
             lambda: hip.mesh_shade(v, f, face, bary[:-2], view, out=guards["rgba"].t),
             lambda: hip.mesh_shade(v, f, face.float(), bary, view, out=guards["rgba"].t),
             lambda: hip.mesh_shade(v, f, face.view(-1), bary, view, out=guards["rgba"].t),
             lambda: hip.mesh_shade(v, f, face, bary, view, out=guards["rgba"].t[:-4])]
    for call in wrong:
        with pytest.raises(hip.MnerfError):
            call()
    torch.cuda.synchronize()
    assert all(g.untouched() and bool((g.t == g.value).all()) for g in guards.values()) and mesh.unwritten()  # nothing was written
    hip.mesh_raster(v, f, view, (h, w), legacy=False, out=out)  # the same call without a flaw writes
    hip.mesh_shade(v, f, face, bary, view, atlas=a, block=block, out=guards["rgba"].t)
    torch.cuda.synchronize()
    assert bool((face >= 0).any()) and bool((guards["rgba"].t.view(h, w, 4)[..., 3] == 1).any()) and all(g.untouched() for g in guards.values())
