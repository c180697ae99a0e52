"""Geometry export on the GPU (matchnerf_amd/csrc/fusion.hip): the consistency kernel against the float64 restatement of
tests/fusion_helpers.py on the analytic scene, the stable compaction against the numpy selection, the colour map byte for byte, and
the host paths (MatchNeRF.export_points, Coach.export_geometry, vis_depth).

Gates.  n_consistent: equal on every pixel the restatement does not mark borderline (at most 1 % of a case's pixels, asserted).
Fused depth where the counts agree: relative error below the larger of 1e-5 and 8 x the error of the same restatement run in fp32,
that error itself below 1e-5 (the gate form of tests/test_ray_chunk_backward_gpu.py).  Point rows: rgb, d, n bit-equal, xyz within
1e-5 of the largest coordinate.  Colour map: equal bytes."""
import numpy as np
import pytest
import torch

import fusion_helpers as F

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


# ------------------------------------------------------------------------------------------------ a. consistency
@pytest.mark.parametrize("k,h,w,legacy", F.GPU_CASES)
def test_consistency_against_float64(hip, k, h, w, legacy):
    worst = {}
    for variant in (F.VARIANTS if k == 3 else ("plain",)):
        s, refs = F.scene(k, h, w, legacy, variant), F.reference(k, h, w, legacy, variant)
        views = _views(hip, s["cams"])
        depth = torch.from_numpy(s["depth"]).cuda()
        opacity = None if s["opacity"] is None else torch.from_numpy(s["opacity"]).cuda()
        left_out, err, e32 = 0, 0.0, 0.0
        for ref in range(k):
            fbuf, fused = _guarded(h * w)
            cbuf, count = _guarded(h * w, torch.int32, -777)
            hip.depth_consistency(views, ref, depth, opacity, legacy=legacy, px_tol=F.PX_TOL, rel_tol=F.REL_TOL,
                                  min_opacity=F.MIN_OPACITY, out=(fused, count))
            torch.cuda.synchronize()
            assert _guards_untouched(fbuf, h * w) and _guards_untouched(cbuf, h * w, -777), (variant, ref)
            got_f, got_c = fused.cpu().numpy().reshape(h, w), count.cpu().numpy().reshape(h, w)
            want = refs[ref]
            keep = ~want["border"]
            left_out += int(want["border"].sum())
            assert np.array_equal(got_c[keep], want["count"][keep]), (variant, ref, np.argwhere((got_c != want["count"]) & keep)[:5])
            invalid = keep & (want["fused"] == 0)  # an invalid reference pixel: 0 and 0.0 exactly
            assert (got_c[invalid] == 0).all() and (got_f[invalid] == 0).all(), (variant, ref)
            same = (got_c == want["count"]) & (want["fused"] > 0)
            same32 = (want["count32"] == want["count"]) & (want["fused"] > 0)
            err = max(err, float((np.abs(got_f - want["fused"])[same] / want["fused"][same]).max()))
            e32 = max(e32, float((np.abs(want["fused32"] - want["fused"])[same32] / want["fused"][same32]).max()))
        print(f"fusion consistency K={k} {h}x{w} legacy={legacy} {variant}: fused depth rel err {err:.3e} (fp32 restatement {e32:.3e}), "
              f"{left_out} of {k * h * w} pixels borderline")
        assert left_out <= F.BORDERLINE_CAP * k * h * w, (variant, left_out)
        assert e32 < 1e-5 and err < max(1e-5, 8 * e32), (variant, err, e32)
        worst[variant] = err
    assert worst


def test_consistency_runs_are_identical_and_opacity_one_is_no_opacity(hip):
    k, h, w = 5, 24, 32
    s = F.scene(k, h, w, False)
    views, depth = _views(hip, s["cams"]), torch.from_numpy(s["depth"]).cuda()
    a = hip.depth_consistency(views, 2, depth, None, legacy=False)
    b = hip.depth_consistency(views, 2, depth, None, legacy=False)
    c = hip.depth_consistency(views, 2, depth, torch.ones_like(depth), legacy=False)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and all(torch.equal(x, y) for x, y in zip(a, c))
    assert int(a[1].max()) == k - 1  # some pixel is seen consistently by every partner


# ------------------------------------------------------------------------------------------------ b. point cloud
TILE_PIXELS = 256 * 1024  # what ONE workgroup of the scan covers: 1024 workgroup counts of 256 pixels
# (h, w): one wave and its neighbours, one workgroup and its neighbours, an odd frame, and the first sizes at which the scan of the
# workgroup counts takes a second workgroup (1025 counts) - as a single row and as a frame of two rows
CLOUD_SIZES = [(1, 1), (1, 63), (1, 64), (1, 65), (1, 255), (1, 257), (37, 53), (1, TILE_PIXELS), (1, TILE_PIXELS + 1),
               (2, TILE_PIXELS // 2 + 1)]
MIN_CONSISTENT = 2


def _cloud_inputs(h, w, mask):
    rng = np.random.default_rng(h * 7919 + w)
    n = h * w
    cam = F.arc_cameras(3, h, w)[1]
    depth = rng.uniform(1.0, 4.0, n).astype(np.float32)
    rgb = rng.random((n, 3)).astype(np.float32)
    count = dict(all=np.full(n, 3), none=np.full(n, MIN_CONSISTENT - 1), alternating=np.where(np.arange(n) % 2 == 0, 2, 1),
                 random=rng.integers(0, 5, n))[mask].astype(np.int32)
    if mask == "random":  # the depth's own part of the selection: non-finite and non-positive values
        for value in (np.nan, np.inf, -np.inf, 0.0, -2.0):
            depth[rng.random(n) < 0.02] = np.float32(value)
    return cam, depth, rgb, count


@pytest.mark.parametrize("mask", ["all", "none", "alternating", "random"])
@pytest.mark.parametrize("h,w", CLOUD_SIZES)
def test_point_cloud_is_the_numpy_selection_in_pixel_order(hip, h, w, mask):
    n = h * w
    cam, depth, rgb, count = _cloud_inputs(h, w, mask)
    legacy = (h + w) % 2 == 0
    view = hip.make_view(cam["extr"], cam["intr"], cam["near"], cam["far"])
    idx, want = F.point_rows(cam, h, w, legacy, depth, rgb, count, MIN_CONSISTENT)
    d_dev, rgb_dev, cnt_dev = torch.from_numpy(depth).cuda(), torch.from_numpy(rgb).cuda(), torch.from_numpy(count).cuda()

    def run(capacity):
        buf = torch.full((capacity + GUARD, 8), SENTINEL, device="cuda")
        total = torch.full((1,), -5, dtype=torch.int64, device="cuda")
        hip.point_cloud(view, (h, w), d_dev, rgb_dev, cnt_dev, MIN_CONSISTENT, legacy=legacy, points=buf[:capacity], count=total)
        return buf, int(total)

    buf, total = run(n)
    assert total == len(idx)
    assert bool((buf[total:] == SENTINEL).all())  # nothing beyond the selected rows, the guard included
    assert mask != "none" or total == 0
    if total == 0:  # nothing was written at all
        return
    got = buf[:total].cpu().numpy()
    assert np.array_equal(got[:, 3].view(np.int32), depth[idx].view(np.int32))
    assert np.array_equal(got[:, 4:7].view(np.int32), rgb[idx].view(np.int32))
    assert np.array_equal(got[:, 7], count[idx].astype(np.float32))
    assert np.abs(got[:, :3] - want[:, :3]).max() <= 1e-5 * np.abs(want[:, :3]).max()
    again, total2 = run(n)
    assert total2 == total and torch.equal(again, buf)
    capacity = max(total // 2, 1) if total > 1 else 0  # fewer rows than selected
    small, total3 = run(capacity)
    assert total3 == total and torch.equal(small[:capacity], buf[:capacity]) and bool((small[capacity:] == SENTINEL).all())


def test_fuse_joins_the_views_in_order(hip):
    """fusion.fuse on the analytic scene: the rows of view k are the compaction of view k's consistency result, view after view; and
    with more views than a launch takes, every view is checked against its 15 nearest"""
    from matchnerf_amd import fusion
    k, h, w = 5, 24, 32
    s, refs = F.scene(k, h, w, False), F.reference(k, h, w, False)
    views, depth = _views(hip, s["cams"]), torch.from_numpy(s["depth"]).cuda()
    rgb = torch.rand(k, h * w, 3, device="cuda")
    cloud, rows = fusion.fuse(views, depth, None, rgb, (h, w), False, return_counts=True)
    assert cloud.shape == (sum(rows), 8) and torch.equal(cloud, fusion.fuse(views, depth, None, rgb, (h, w), False))
    at = 0
    for ref in range(k):
        keep = ~refs[ref]["border"].reshape(-1)
        want = (refs[ref]["count"].reshape(-1) >= 2)
        fused, cnt = hip.depth_consistency(views, ref, depth, None, legacy=False)
        sel = (cnt.reshape(-1) >= 2) & (fused.reshape(-1) > 0)
        assert rows[ref] == int(sel.sum()) and np.array_equal(sel.cpu().numpy()[keep], want[keep])
        part = cloud[at:at + rows[ref]]
        assert torch.equal(part[:, 3], fused.reshape(-1)[sel]) and torch.equal(part[:, 4:7], rgb[ref][sel])
        at += rows[ref]
    # the planted outliers of view 0 are gone, the surfaces are there: every point lies on the plane or on the box in front of it
    xyz = cloud[:, :3].cpu().numpy()
    assert rows[0] <= (~s["outliers"]).sum() and -0.61 < xyz[:, 2].min() and xyz[:, 2].max() < 0.01
    # 18 views: more than one launch takes
    k = 18
    cams = F.arc_cameras(k, h, w)
    depth = torch.from_numpy(np.stack([F.raycast(c, h, w, False) for c in cams]).astype(np.float32)).cuda()
    views = _views(hip, cams)
    rgb = torch.rand(k, h * w, 3, device="cuda")
    cloud, rows = fusion.fuse(views, depth, None, rgb, (h, w), False, return_counts=True)
    centres = fusion.camera_centres(views)
    for ref in (0, 9, 17):
        group = sorted(fusion.partners_of(centres, ref) + [ref])
        assert len(group) == 16
        fused, cnt = hip.depth_consistency([views[j] for j in group], group.index(ref), depth[group].contiguous(), None, legacy=False)
        assert rows[ref] == int(((cnt >= 2) & (fused > 0)).sum()) > 0


# ------------------------------------------------------------------------------------------------ c. colour map
def test_colormap_bytes(hip):
    lo, hi = 2.0, 6.0
    index = np.arange(256)
    ramp = (lo + (index + 0.5) / 255.0 * (hi - lo)).astype(np.float32)  # mid-points: every index once, far from a truncation edge
    got = hip.depth_colormap(torch.from_numpy(ramp).cuda(), lo, hi).cpu().numpy()
    assert np.array_equal(got, F.colormap(ramp, lo, hi)) and len(np.unique(got, axis=0)) == 256
    edge = np.array([np.nan, 0.0, lo - 1.0, lo, hi, hi + 100.0, np.inf, -np.inf, 3.0e38, -3.0e38], np.float32)
    # (in the header's fp32 arithmetic: hi - lo + 1e-8 rounds to hi - lo, so hi itself reaches index 255, as in the reference's
    # float32 numpy; float64 would stop at 254)
    got = hip.depth_colormap(torch.from_numpy(edge).cuda(), lo, hi).cpu().numpy()
    assert np.array_equal(got, F.colormap(edge, lo, hi, dtype=np.float32))
    assert np.array_equal(np.delete(got, 4, 0), np.delete(F.colormap(edge, lo, hi), 4, 0))  # float64 agrees everywhere else
    # a frame of arbitrary depths: the device's operations are the restatement's, one rounding each, in float32
    frame = np.random.default_rng(3).uniform(1.0, 7.0, (37, 53)).astype(np.float32)
    frame[3, 4:9] = np.nan
    buf, out = _guarded(37 * 53 * 3, torch.uint8, 77)
    got = hip.depth_colormap(torch.from_numpy(frame).cuda(), lo, hi, out=out)
    torch.cuda.synchronize()
    assert _guards_untouched(buf, 37 * 53 * 3, 77)
    assert np.array_equal(got.cpu().numpy().reshape(37, 53, 3), F.colormap(frame, lo, hi, dtype=np.float32))
    assert hip.depth_colormap(torch.empty(0, device="cuda"), lo, hi).shape == (0, 3)  # n = 0


# ------------------------------------------------------------------------------------------------ the module
# random weights render no surface: the thresholds are opened so that rows come out at all; the bookkeeping under test (one encoder
# pass, masks -> rows, every row at its own pixel and depth, determinism) does not depend on which pixels survive
LOOSE = dict(px_tol=64.0, rel_tol=0.9, min_opacity=0.01, min_consistent=1)


def _model(name):
    from helpers import golden_case
    from test_model_gpu import build_model, to_batch
    g, *_ = golden_case(name)
    opt, model = build_model(g["meta"])
    calls = []
    encode = model.get_img_feat
    model.get_img_feat = lambda *a, **k: (calls.append(1), encode(*a, **k))[1]
    return opt, model, to_batch(g), calls


@pytest.mark.parametrize("name", ["c1_default", "nonlegacy"])
def test_export_points_rows_are_the_masks(hip, name):
    opt, model, batch, calls = _model(name)
    legacy = bool(opt.nerf.legacy_coord)
    with torch.no_grad():
        clouds, maps = model.export_points(batch, views="sources", return_maps=True, **LOOSE)
        assert len(calls) == 1  # one encoder pass for the K renders
        again = model.export_points(batch, views="sources", **LOOSE)
        default = model.export_points(batch)  # the shipped thresholds: whatever survives, the call returns rows of 8
    assert len(calls) == 3 and len(clouds) == 1 and torch.equal(clouds[0], again[0]) and default[0].shape[1] == 8
    cloud, (h, w), k = clouds[0], maps.hw, model.n_src_views
    assert (h, w) == tuple(batch.images.shape[-2:]) and maps.depth.shape == (1, k, h, w) and cloud.shape[1] == 8
    rows, at = maps.counts[0], 0
    assert sum(rows) == cloud.shape[0] > 0
    cams = [dict(extr=np.array(list(v.extr), np.float32).reshape(3, 4), intr=np.array(list(v.intr), np.float32).reshape(3, 3))
            for v in maps.views[0]]
    inv = F.inverse_cameras(cams, np.float64)
    off = 0.0 if legacy else 0.5
    for ref in range(k):  # stage by stage: consistency -> mask -> the view's rows
        fused, cnt = hip.depth_consistency(maps.views[0], ref, maps.depth[0], maps.opacity[0], legacy=legacy, px_tol=LOOSE["px_tol"],
                                           rel_tol=LOOSE["rel_tol"], min_opacity=LOOSE["min_opacity"])
        sel = ((cnt >= LOOSE["min_consistent"]) & torch.isfinite(fused) & (fused > 0)).reshape(-1)
        assert rows[ref] == int(sel.sum())
        part = cloud[at:at + rows[ref]].cpu().numpy().astype(np.float64)
        at += rows[ref]
        idx = torch.nonzero(sel).reshape(-1).cpu().numpy()
        u, v, z = F.proj(inv[ref], part[:, :3])  # every row at its own pixel centre and depth
        assert np.abs(u - (idx % w + off)).max() < 1e-3 and np.abs(v - (idx // w + off)).max() < 1e-3
        assert (np.abs(z - part[:, 3]) <= 1e-5 * np.abs(part[:, 3])).all()
        assert np.array_equal(part[:, 3].astype(np.float32), fused.reshape(-1)[sel].cpu().numpy())
        assert np.array_equal(part[:, 4:7].astype(np.float32), maps.rgb[0, ref][sel].cpu().numpy())
        assert np.array_equal(part[:, 7], cnt.reshape(-1)[sel].cpu().numpy().astype(np.float64))


def test_export_points_along_the_video_path_and_from_pose_dicts(hip):
    opt, model, batch, calls = _model("nonlegacy")
    opt.nerf.video_n_frames = 6  # (the interpolated path has n // 3 poses per leg)
    with torch.no_grad():
        clouds, maps = model.export_points(batch, views="path", return_maps=True, **LOOSE)
        tgt, ref = model.extract_poses(batch)
        poses = [tgt] + [dict(extrinsics=ref["extrinsics"][:, v], intrinsics=ref["intrinsics"][:, v], near_fars=ref["near_fars"][:, v])
                         for v in range(2)]
        listed = model.export_points(batch, views=poses, **LOOSE)
    assert len(calls) == 2 and maps.depth.shape[1] == 6 and len(maps.counts[0]) == 6 and clouds[0].shape == (sum(maps.counts[0]), 8)
    assert listed[0].shape[1] == 8 and listed[0].shape[0] > 0


def test_export_points_refusals_precede_any_launch(hip):
    opt, model, batch, calls = _model("nonlegacy")
    with pytest.raises(NotImplementedError):  # gradients
        model.export_points(batch)
    with torch.no_grad():
        from matchnerf_amd.edict import EasyDict
        with pytest.raises(ValueError, match="pinhole"):
            model.export_points(EasyDict(dict(batch, tgt_camera="fisheye")))
        with pytest.raises(TypeError):
            model.export_points(batch, tolerance=1.0)
        opt.nerf.depth.param = "inverse"
        with pytest.raises(ValueError, match="inverse"):
            model.export_points(batch)
    assert calls == []  # not even the encoder ran


# ------------------------------------------------------------------------------------------------ the coach
def _coach(tmp_path, monkeypatch, *extra):
    from matchnerf_amd import options
    from matchnerf_amd.coach import Coach
    monkeypatch.chdir(tmp_path)
    cmd = options.parse_arguments(["--yaml=test", "--name=geometry", "--nerf.sample_intvs=16", "--data_test.llff=", "--data_test.blender=",
                                   "--data_test.tnt=", "--data_test.dtu.img_wh=48,32", "--data_test.dtu.max_len=1",
                                   "--nerf.video_n_frames=3", "--nerf.save_frames"] + list(extra))
    c = Coach(options.set(cmd, verbose=False))
    c.build_networks()
    c.restore_checkpoint()
    c.load_dataset()
    return c


def test_coach_export_geometry_writes_ply_and_depth_maps(tmp_path, monkeypatch):
    from PIL import Image
    c = _coach(tmp_path, monkeypatch, "--nerf.export_geometry=sources", "--nerf.fuse_px_tol=64", "--nerf.fuse_rel_tol=0.9",
               "--nerf.fuse_min_opacity=0.01", "--nerf.fuse_min_views=1", "--vis_depth")
    written = c.export_geometry()
    assert list(written) == ["dtu"] and len(written["dtu"]) == 1 and written["dtu"][0].endswith(".ply")
    xyz, rgb = F.read_ply(written["dtu"][0])  # (the reader asserts header count == rows)
    assert len(xyz) > 0 and np.isfinite(xyz).all() and rgb.std() > 0
    out_dir = tmp_path / "outputs" / "geometry" / "geometry" / "dtu"
    panels = sorted(out_dir.glob("*_depth*.png"))
    assert len(panels) == 3
    for p in panels:
        with Image.open(p) as im:
            assert im.size == (48, 32) and im.mode == "RGB"
    c.opts.vis_depth = False  # without it: the cloud alone, the same bytes
    before = open(written["dtu"][0], "rb").read()
    for p in panels:
        p.unlink()
    assert c.export_geometry("sources") == written and open(written["dtu"][0], "rb").read() == before
    assert not list(out_dir.glob("*_depth*.png"))


def test_vis_depth_panels_in_video_and_test_strips(tmp_path, monkeypatch, hip):
    from PIL import Image
    c = _coach(tmp_path, monkeypatch)
    assert not c.opts.vis_depth
    off = c.test_model_video()["dtu"]  # the option off: the parent's code path
    frames_dir = tmp_path / "outputs" / "geometry" / "test_videos" / "dtu"
    off_files = {p.name: p.read_bytes() for p in sorted(frames_dir.glob("*_f*.jpg"))}
    assert off.shape == (3, 32, 48, 3) and len(off_files) == 3
    c.opts.vis_depth = True
    with pytest.warns(UserWarning, match="mp4"):
        on = c.test_model_video()["dtu"]
    assert on.shape == (3, 32, 96, 3) and on.dtype == np.uint8
    assert np.array_equal(on[:, :, :48], off)  # rgb | depth: the left half is the frame, byte for byte
    assert on[:, :, 48:].std() > 0
    for p in sorted(frames_dir.glob("*_f*.jpg")):
        with Image.open(p) as im:
            assert im.size == (96, 32)
    c.opts.vis_depth = False  # and off again: the files of the first run, byte for byte
    again = c.test_model_video()["dtu"]
    assert np.array_equal(again, off) and {p.name: p.read_bytes() for p in sorted(frames_dir.glob("*_f*.jpg"))} == off_files
    # test strips: pred | gt without, depth | pred | gt with
    strips = tmp_path / "outputs" / "geometry" / "test"
    c.test_model(save_images=True)
    plain = {p.name: p.read_bytes() for p in strips.glob("*.png")}
    c.opts.vis_depth = True
    c.test_model(save_images=True)
    assert len(plain) == 1
    for name, data in plain.items():
        with Image.open(strips / name) as im:
            wide = np.asarray(im)
        import io
        narrow = np.asarray(Image.open(io.BytesIO(data)))
        assert narrow.shape == (32, 96, 3) and wide.shape == (32, 144, 3) and np.array_equal(wide[:, 48:], narrow)
        # the depth panel is the device colour map of the rendered depth between the target's near and far
        assert wide[:, :48].std() > 0
