"""MatchNeRF — drop-in module for the reference's ``models.matchnerf.MatchNeRF``.

Same constructor (``MatchNeRF(opts)``), same attributes (``feat_enc``, ``nerf_dec``,
``nerf_setbg_opaque``, ``n_src_views``), same ``forward(batch, mode, render_video,
render_path_mode)`` contract and the same ``state_dict`` keys as
/root/reference/models/matchnerf.py:13-325 — but the per-ray hot path runs in hand-written
HIP kernels for MI355X (``libmnerf_hip.so``, include/mnerf.h):

    encoder        GMFlow with the K6 shifted-window attention kernel        (gmflow.py)
    render chunk   K1+K2 cost volume -> K3+K4+K5 fused decoder/compositing   (mnerf_render_chunk)

What the reference does per 4096-ray chunk in ~100 eager ops (full-image ray grid, six
268 MB sampled-feature tensors, [R,4,S,S] attention scores ...) is two kernel launches here,
fed by pair-major channel-last feature maps that stay resident in HBM for the whole frame.

The HIP path is the ONLY path: there is no eager fallback.  Without the shared library or
without a GPU, rendering raises ``hip.MnerfError`` / ``RuntimeError``.

Every inference path (pixel rays, ray bundles, pose tables) takes its scenes from ONE per-source-set context
(``SourceSet``, through ``MatchNeRF._sources``) and walks batch elements and ray chunks in ONE loop (``launch_chunks``).
"""
import os

import numpy as np
import torch

from . import camera, hip
from .cond_nerf import CondNeRF
from .edict import EasyDict as edict
from .gmflow import GMFlow, pair_major_to_view_chunks

# rays per kernel launch when a full image is rendered.  The reference's
# ``nerf.rand_rays_{val,test}`` only bounds its temporaries (README.md:132); results are
# chunk-invariant (tests/test_hip_kernels.py), so larger launches are used here.
MAX_RAYS_PER_LAUNCH = int(os.environ.get("MNERF_MAX_RAYS_PER_LAUNCH", "65536"))
# a pose-table launch (render_poses) may carry more: frames of a video are rendered back to back anyway, and with 288 GB of HBM
# the conditioning hand-off of a quarter of a million rays (3 GB at 128 samples per ray) is no constraint.  What it buys is fewer,
# fuller launches: configs/demo_own.yaml's 24 frames of 256 x 160 at S = 128 go out as 4 launches of 6 poses instead of 24 x 2.
MAX_RAYS_PER_POSE_LAUNCH = int(os.environ.get("MNERF_MAX_RAYS_PER_POSE_LAUNCH", "262144"))
# rays per autograd node when gradients are required (bounds the temporaries of the re-evaluated backward)
GRAD_RAYS_PER_CALL = 8192


def launch_chunks(batch_size, n_rays, chunk, device, launch):
    """The one batch-by-chunk loop of the render paths: allocates rgb [B,n_rays,3], depth [B,n_rays,1], opacity [B,n_rays,1] on
    ``device`` and calls ``launch(b, first, count, rgb, depth, opacity)`` - the last three are the [count, C] slices of element b
    to write - for every batch element and every run of at most ``chunk`` rays, in increasing order.  No rays: empty outputs and no
    call, so a caller that builds scenes, operand images and workspaces from inside ``launch`` builds none."""
    out = edict(rgb=torch.empty(batch_size, n_rays, 3, device=device), depth=torch.empty(batch_size, n_rays, 1, device=device),
                opacity=torch.empty(batch_size, n_rays, 1, device=device))
    for b in range(batch_size):
        for c in range(0, n_rays, chunk):
            m = min(chunk, n_rays - c)
            launch(b, c, m, out.rgb[b, c:c + m], out.depth[b, c:c + m], out.opacity[b, c:c + m])
    return out


class SourceSet:
    """Launch context of one source set, built once and shared by every target pose rendered from it (all frames of a video, all
    chunks of a frame): host copies of the source cameras (they travel by value in the kernel arguments), the channel-last RGBA
    copy of the source images and, per batch element on first use, the ``hip.Scene`` and - for a matrix-form launch - the
    split-fp16 operand image of the feature maps (``hip.cost_volume_operands``: two short launches, ~the bytes of the maps).
    ``key`` is the identity, version and shape of ``keyed`` = (images, extrinsics, intrinsics, near_fars, *feature maps), so
    in-place edits or a new batch rebuild the context; it holds the keyed tensors themselves, so their storage cannot be freed and
    handed to a NEW batch at the same address while it lives (the caching allocator does exactly that in the reference's coach
    loop), and ``forward`` drops it at its top: a context is shared by the poses and chunks of ONE forward, never by two batches."""

    def __init__(self, key, keyed, n_views, groups):
        self.key, self.keyed, self.n_views = key, keyed, n_views
        ref_images, self.feats = keyed[0], list(keyed[4:])
        self.groups = [groups] if isinstance(groups, int) else list(groups)
        self.host = tuple(MatchNeRF._host(t) for t in keyed[1:4])  # extrinsics [B,V,3,4], intrinsics [B,V,3,3], near_fars [B,V,2]
        b, v, _, h, w = ref_images.shape
        self.images_cl = torch.zeros(b, v, h, w, 4, device=ref_images.device)
        self.images_cl[..., :3] = ref_images.detach().permute(0, 1, 3, 4, 2)
        self._scenes, self._ops = {}, {}

    def build(self, b, feats_b):
        """A fresh ``hip.Scene`` of batch element b over the per-scale maps ``feats_b`` [P,2,h,w,128] (the cached scenes pass
        slices of the keyed maps, the training path the tensors autograd hands it)."""
        sc = hip.Scene()
        sc.n_views, sc.n_scales = self.n_views, len(feats_b)
        assert len(self.groups) == len(feats_b), "cos_n_group needs one entry per feature scale"
        for s, f in enumerate(feats_b):
            assert f.is_contiguous()
            sc.fh[s], sc.fw[s] = f.shape[2], f.shape[3]
            sc.n_group[s] = self.groups[s]
            sc.feat[s] = f.data_ptr()
        sc.images = self.images_cl[b].data_ptr()
        ex, it, nf = self.host
        for v in range(self.n_views):
            sc.views[v] = hip.make_view(ex[b, v], it[b, v], nf[b, v, 0], nf[b, v, 1])
        return sc

    def scene(self, b, matrix_form=False):
        """The scene of batch element b, built on first use.  ``matrix_form``: the one whose ``feat_op`` names the operand image,
        which sends the cost volume to the matrix pipe; without it a struct of its own, whose ``feat_op`` stays unset (the walk)."""
        if (b, matrix_form) not in self._scenes:
            sc = self._scenes[b, matrix_form] = self.build(b, [f[b] for f in self.feats])
            if matrix_form:
                self._ops[b] = hip.cost_volume_operands(sc, device=self.feats[0].device)
        return self._scenes[b, matrix_form]


class MatchNeRF(torch.nn.Module):
    def __init__(self, opts):
        super().__init__()
        self.opts = opts
        self.nerf_setbg_opaque = False
        self.n_src_views = opts.n_src_views
        if self.n_src_views > hip.MNERF_MAX_VIEWS:
            raise NotImplementedError(f"n_src_views={self.n_src_views} > {hip.MNERF_MAX_VIEWS}")
        self.feat_enc = GMFlow(feature_channels=128, num_scales=1, num_head=1, attention_type="swin",
                               ffn_dim_expansion=4, feature_upsampler=opts.encoder.feature_upsampler,
                               upsample_factor=opts.encoder.upsample_factor,
                               num_transformer_layers=opts.encoder.num_transformer_layers,
                               device=opts.device).to(opts.device)
        self.nerf_dec = CondNeRF(opts).to(opts.device)
        if getattr(opts.encoder, "feature_sample_local_radius", 0):
            raise NotImplementedError("encoder.feature_sample_local_radius > 0 (gmflow/utils.py:136-162) is not "
                                      "built; every shipped config uses 0 (base.yaml:27)")
        self._ws = None
        self._enc_graphs = {}     # captured encoder passes (get_img_feat), keyed by input shape and weight versions
        self.encoder_graph = os.environ.get("MNERF_ENCODER_GRAPH", "0") == "1"  # opt-in: measured no gain (see _encoder_graph_replay)
        self._src = None          # the SourceSet of the forward in flight: see _sources
        self.kernel_timer = None  # hip.KernelTimer: per-kernel event timing (bench.py)
        self.fused_render = False  # True: ray chunks take the one-launch form where it exists (slower on MI355X: DESIGN.md)
        # video of small frames: several poses per launch through a pose table (mnerf_rays.pose_table).  OFF by default since
        # round 6: the table never paid (157.4 against 158.6 ms for demo_own.yaml's 24 frames, profiles/history/r5_video_demo_own.log)
        # and it keeps the cost volume on the segment walk, which the matrix form of the pose-by-pose launches now beats
        # (DESIGN.md section 4).  MNERF_POSE_BATCHING=1 brings it back; tests/test_pose_table_gpu.py keeps it bit-identical.
        self.pose_batching = os.environ.get("MNERF_POSE_BATCHING", "0") == "1"
        self.cv_matrix_form = os.environ.get("MNERF_CV_MM", "1") != "0"  # full-frame renders: the cost volume on the matrix pipe

    def _dec(self):
        """the CondNeRF module, also when the reference's coach wrapped it in nn.DataParallel (coach.py:83-85)"""
        return getattr(self.nerf_dec, "module", self.nerf_dec)

    # ------------------------------------------------------------------ forward (matchnerf.py:32-73)
    def forward(self, batch, mode=None, render_video=False, render_path_mode="interpolate"):
        self._src = None  # the launch context never outlives one forward (see SourceSet)
        ref_images = batch.images[:, :self.n_src_views]
        tgt_pose, ref_poses = self.extract_poses(batch)
        batch_size, _, _, img_h, img_w = ref_images.shape
        tgt_pose, tgt_hw, ssaa = self.target_grid(batch, mode, tgt_pose, (img_h, img_w))  # the outputs are [B, h*w, C] of this grid
        if mode == "train" and (tgt_hw != (img_h, img_w) or ssaa != 1):  # (before the first launch)
            raise NotImplementedError(f"mode='train' renders at the views' size {(img_h, img_w)}, not at {tgt_hw} x ssaa {ssaa}: "
                                      "the ground truth has the batch's size")
        tgt_camera = self.target_camera(batch, mode)  # None: the batch's pinhole camera, today's path
        if tgt_camera is not None and mode == "train":  # (before the first launch)
            raise NotImplementedError(f"a {tgt_camera['model']} target camera renders caller-supplied rays, which are inference only "
                                      f"(mode={mode!r})")
        ref_feats_list = self.get_img_feat(ref_images, attn_splits_list=self.opts.encoder.attn_splits_list,
                                           cur_n_src_views=self.n_src_views)

        if render_video:
            assert mode in ["test", "val"], f"Do NOT render video in mode {mode}, change to either 'test' or 'val'."
            poses_paths = self.get_video_rendering_path(tgt_pose, ref_poses, render_path_mode,
                                                        self.opts.nerf.video_n_frames, batch)
        else:
            poses_paths = [tgt_pose]

        mode_rand_rays = getattr(self.opts.nerf, f"rand_rays_{mode}", 0)
        collected, frames_done = {}, {}
        if render_video and self.pose_batching:
            # small frames: as many poses per launch as fill one (mnerf_rays.pose_table); None where the kernels or the
            # frame size do not take a table -> the pose loop below
            # (a pose table holds pinhole constants: another camera model goes pose by pose through its ray bundle)
            frames = None if (ssaa > 1 or tgt_camera is not None) else self.render_poses(self.opts, poses_paths, ref_poses=ref_poses, ref_images=ref_images,
                                                             ref_feats_list=ref_feats_list, tgt_hw=tgt_hw)
            if frames is not None:
                for k, v in frames.items():  # [n_poses, B, N, C] -> the reference's frame-major [n_poses * B, N, C]
                    host = torch.empty((v.shape[0] * v.shape[1],) + tuple(v.shape[2:]), dtype=v.dtype, pin_memory=True)
                    host.copy_(v.reshape(host.shape), non_blocking=True)
                    collected[k] = host
                    frames_done[k] = v
                poses_paths = []
        for cur_tgt_pose in poses_paths:
            if tgt_camera is not None:
                ret = self.render_camera(self.opts, cur_tgt_pose, tgt_camera, tgt_hw, ssaa=ssaa, mode=mode, ref_poses=ref_poses,
                                         ref_images=ref_images, ref_feats_list=ref_feats_list)
            elif mode_rand_rays and mode in ["train", "test-optim"]:
                batch.ray_idx = torch.randperm(img_h * img_w, device=ref_images.device)[:mode_rand_rays // batch_size]
                ret = self.render(self.opts, cur_tgt_pose, ray_idx=batch.ray_idx, mode=mode, ref_poses=ref_poses,
                                  ref_images=ref_images, ref_feats_list=ref_feats_list, tgt_hw=tgt_hw, ssaa=ssaa)
            elif mode_rand_rays:
                ret = self.render_by_slices(self.opts, cur_tgt_pose, mode=mode, ref_poses=ref_poses,
                                            ref_images=ref_images, ref_feats_list=ref_feats_list, tgt_hw=tgt_hw, ssaa=ssaa)
            else:
                ret = self.render(self.opts, cur_tgt_pose, mode=mode, ref_poses=ref_poses, ref_images=ref_images,
                                  ref_feats_list=ref_feats_list, tgt_hw=tgt_hw, ssaa=ssaa)
            if render_video:
                # Frames go to the host as the reference's do (matchnerf.py:62-70, per-frame .cpu()), but without a
                # host sync per frame: one pinned buffer per output holds all frames, each frame is an async copy
                # queued behind its own kernels, and the GPU starts the next pose while Python is still here.
                for k, v in ret.items():
                    v = v.detach()
                    if k not in collected:
                        collected[k] = torch.empty((len(poses_paths) * v.shape[0],) + tuple(v.shape[1:]), dtype=v.dtype,
                                                   pin_memory=True)
                    lo = len(frames_done.setdefault(k, [])) * v.shape[0]
                    collected[k][lo:lo + v.shape[0]].copy_(v, non_blocking=True)
                    frames_done[k].append(v)  # keep the device tensor alive until the copy has run
            else:
                for k, v in ret.items():
                    collected.setdefault(k, []).append(v)
        if render_video:
            torch.cuda.current_stream(ref_images.device).synchronize()
            for k, v in collected.items():
                batch[k] = v
        else:
            for k, v in collected.items():
                batch[k] = torch.cat(v, dim=0)
        return batch

    def extract_poses(self, batch):
        """matchnerf.py:75-86: target = LAST view, sources = all the others."""
        tgt_pose = dict(extrinsics=batch.extrinsics[:, -1, :3, :], intrinsics=batch.intrinsics[:, -1],
                        near_fars=batch.near_fars[:, -1])
        ref_poses = dict(extrinsics=batch.extrinsics[:, :-1, :3, :], intrinsics=batch.intrinsics[:, :-1],
                         near_fars=batch.near_fars[:, :-1])
        return tgt_pose, ref_poses

    # ------------------------------------------------------------------ target grid
    @staticmethod
    def resize_pose(pose, src_hw, tgt_hw, legacy):
        """``pose`` (dict of extrinsics / intrinsics / near_fars [+ "_host"]) with its intrinsics moved from a ``src_hw`` frame to
        a ``tgt_hw`` frame of the same field of view (``camera.resize_intrinsics``)."""
        if tuple(src_hw) == tuple(tgt_hw):
            return pose
        out = dict(pose)
        out["intrinsics"] = camera.resize_intrinsics(pose["intrinsics"], src_hw, tgt_hw, legacy)
        if "_host" in pose:
            ex, it, nf = pose["_host"]
            out["_host"] = (ex, camera.resize_intrinsics(it, src_hw, tgt_hw, legacy), nf)
        return out

    def target_grid(self, batch, mode, tgt_pose, src_hw):
        """The pixel grid the target view is rendered on -> (tgt_pose, (h, w), ssaa).  The source views do not tie it down: the
        radiance field is continuous and the source maps do not depend on the target's grid (mnerf_rays.tgt_height / tgt_width).
          ``batch.tgt_hw`` = (h, w)   the caller's grid; ``batch.intrinsics[:, -1]`` already belongs to it;
          ``nerf.render_hw`` = [h, w] (option, modes 'test' / 'val', when the batch names no grid): the batch's target camera at
                                      another resolution - the intrinsics are ``camera.resize_intrinsics`` of the batch's;
          neither                     the views' size.
        ``ssaa`` (``batch.ssaa``, else the option ``nerf.render_ssaa`` in modes 'test' / 'val'; default 1): ``render`` casts k x k
        rays per pixel and box-filters them on the device."""
        src_hw = (int(src_hw[0]), int(src_hw[1]))
        evaluating = mode in ("test", "val")
        tgt_hw = batch.get("tgt_hw") if hasattr(batch, "get") else None
        if tgt_hw is not None:
            tgt_hw = (int(tgt_hw[0]), int(tgt_hw[1]))
        else:
            opt_hw = getattr(self.opts.nerf, "render_hw", None) if evaluating else None
            if opt_hw:
                if len(opt_hw) != 2:
                    raise ValueError(f"nerf.render_hw={opt_hw!r}: expected height,width")
                tgt_hw = (int(opt_hw[0]), int(opt_hw[1]))
                if tgt_pose is not None:  # (None: the caller only wants the size)
                    tgt_pose = self.resize_pose(tgt_pose, src_hw, tgt_hw, bool(self.opts.nerf.legacy_coord))
            else:
                tgt_hw = src_hw
        ssaa = batch.get("ssaa") if hasattr(batch, "get") else None
        if ssaa is None:
            ssaa = (getattr(self.opts.nerf, "render_ssaa", None) if evaluating else None) or 1
        ssaa = int(ssaa)
        if min(tgt_hw) < 1 or not 1 <= ssaa <= 8:
            raise ValueError(f"target grid {tgt_hw}, ssaa={ssaa}: sizes >= 1 and 1 <= ssaa <= 8")
        return tgt_pose, tgt_hw, ssaa

    def target_camera(self, batch, mode):
        """The camera MODEL of the target view -> None for the batch's pinhole camera (the pixel path), else a dict(model=...,
        fov_deg=..., ortho_width=..., lon_lat=...) for ``camera.camera_model``: ``batch.tgt_camera`` (a dict, or a model name), else
        in modes 'test' / 'val' the options ``nerf.render_camera`` = pinhole | fisheye | sphere | ortho with ``nerf.render_fov``
        (degrees, fisheye / sphere) and ``nerf.render_ortho_width`` (world units, ortho).  The pose, near / far and - for a fisheye
        without a field of view - the intrinsics stay the batch's target view's."""
        spec = batch.get("tgt_camera") if hasattr(batch, "get") else None
        if spec is None and mode in ("test", "val"):
            name = getattr(self.opts.nerf, "render_camera", None)
            if name:
                spec = dict(model=name, fov_deg=getattr(self.opts.nerf, "render_fov", None),
                            ortho_width=getattr(self.opts.nerf, "render_ortho_width", None))
        if spec is None:
            return None
        spec = dict(model=spec) if isinstance(spec, str) else dict(spec)
        if spec.get("model") not in camera.CAMERA_MODELS:
            raise ValueError(f"target camera model {spec.get('model')!r}: one of {camera.CAMERA_MODELS}")
        unknown = set(spec) - {"model", "fov_deg", "ortho_width", "lon_lat"}
        if unknown:
            raise ValueError(f"target camera: unknown keys {sorted(unknown)}")
        return None if spec["model"] == "pinhole" else spec

    # ------------------------------------------------------------------ encoder (matchnerf.py:183-207)
    def get_img_feat(self, imgs, attn_splits_list=None, cur_n_src_views=3):
        """-> list over scales of pair-major channel-last maps [B,P,2,h,w,128]
        (``gmflow.pair_major_to_view_chunks`` converts to the reference's [B,V,(V-1)*128,h,w])."""
        if attn_splits_list is None:
            attn_splits_list = self.opts.encoder.attn_splits_list
        imgs = imgs[:, :cur_n_src_views]
        if self.encoder_graph and imgs.is_cuda and not torch.is_grad_enabled() and not torch.cuda.is_current_stream_capturing():
            return self._encoder_graph_replay(imgs, attn_splits_list)
        return self.feat_enc(imgs=imgs, attn_splits_list=attn_splits_list, wo_self_attn=self.opts.encoder.wo_self_attn)

    def _encoder_graph_replay(self, imgs, attn_splits_list):
        """The inference encoder as ONE HIP graph launch (opt-in: MNERF_ENCODER_GRAPH=1 or .encoder_graph = True).  An encoder
        pass is ~100 short kernels (15 convolutions, 15 norms, 12 x (q|k|v, window attention, K7), layout glue); the idea was
        that launch gaps are a sizeable part of its 3.9 ms.  MEASURED (round 4, same box): frame 30.27-30.50 ms with the graph,
        30.32 without, encoder 3.85 vs 3.89 ms — the host enqueues far enough ahead that the kernels already run back to back;
        what is left of the 3.9 ms is the kernels themselves.  Kept because it is correct and tested, not because it pays.
        Every kernel of the pass is enqueue-only on the current stream (include/mnerf.h), so the
        pass is captured once per (input shape, attention splits, encoder weights) and replayed: the input is copied into the
        graph's static buffer, the outputs are CLONED out of it (78 MB at 3 views: ~40 us), so results never alias a later call.
        A weight update (load_state_dict, an optimizer step) changes the parameters' version counters and thereby the key.
        MNERF_ENCODER_GRAPH=0 (or .encoder_graph = False) keeps the eager pass; a failed capture falls back to it once and
        for all with a warning (the kernels are the same either way)."""
        enc = self.feat_enc
        splits = tuple(attn_splits_list) if isinstance(attn_splits_list, (list, tuple)) else (attn_splits_list,)
        wkey = tuple((int(p._version), int(p.data_ptr())) for p in enc.parameters())
        # what the captured kernels depend on besides the input: the attention arithmetic (MNERF_WA_MATH picks other kernels) and
        # the encoder's tuning knobs; a graph of other WEIGHTS is dead (its key can never match again): dropped, not kept
        shape_key = (tuple(imgs.shape), str(imgs.device), splits, bool(self.opts.encoder.wo_self_attn), hip.wa_math(),
                     os.environ.get("MNERF_WA_MIN4"), os.environ.get("MNERF_WA_XCD"))
        key = shape_key + (hash(wkey),)
        entry = self._enc_graphs.get(key)
        if entry is None:
            for stale in [k for k in self._enc_graphs if k[:-1] == shape_key]:
                del self._enc_graphs[stale]
            run = lambda x: enc(imgs=x, attn_splits_list=attn_splits_list, wo_self_attn=self.opts.encoder.wo_self_attn)
            static_in = imgs.clone()
            run(static_in)  # eager warm-up: weight packing, LDS attributes, cached index / position tensors
            torch.cuda.synchronize(imgs.device)
            try:
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    static_out = run(static_in)
            except Exception as e:  # noqa: BLE001
                import warnings
                warnings.warn(f"encoder graph capture failed ({type(e).__name__}: {e}); using the eager encoder pass")
                self.encoder_graph = False
                return run(imgs)
            if len(self._enc_graphs) >= 4:  # a handful of live shapes at most (each graph owns its activations)
                self._enc_graphs.pop(next(iter(self._enc_graphs)))
            entry = self._enc_graphs[key] = (graph, static_in, static_out)
        graph, static_in, static_out = entry
        static_in.copy_(imgs)
        graph.replay()
        return [o.clone() for o in static_out]

    # ------------------------------------------------------------------ C-ABI argument structs
    def _sources(self, ref_poses, ref_images, ref_feats_list):
        """The ``SourceSet`` of these source views, cameras and feature maps: the cached one while its key matches."""
        keyed = (ref_images, ref_poses["extrinsics"], ref_poses["intrinsics"], ref_poses["near_fars"], *ref_feats_list)
        key = tuple((t.data_ptr(), t._version, tuple(t.shape)) for t in keyed)
        if self._src is None or self._src.key != key:
            self._src = SourceSet(key, keyed, self.n_src_views, self.opts.encoder.cos_n_group)
        return self._src

    def _decoder(self, n_samples, device):
        return self._dec().decoder_struct(n_samples, device, self.nerf_setbg_opaque)

    def _workspace(self, n_floats, device):
        if self._ws is None or self._ws.numel() < n_floats or self._ws.device != device:
            self._ws = torch.empty(n_floats, device=device)
        return self._ws

    @staticmethod
    def _host(t):
        return t.detach().float().cpu().numpy()

    def _needs_grad(self, ref_feats_list):
        return torch.is_grad_enabled() and (any(f.requires_grad for f in ref_feats_list) or
                                            any(p.requires_grad for p in self._dec().parameters()))

    @staticmethod
    def _ray_opts(opt, ref_images, n_samples=None):
        """What every ray struct takes from the options and the source views -> ((n_samples, height, width), dict(legacy=...,
        depth_inverse=...)): the arguments of ``hip.make_rays`` / ``hip.make_free_rays`` after the ray count, and their keywords."""
        n_samples = int(opt.nerf.sample_intvs) if n_samples is None else int(n_samples)
        return (n_samples, ref_images.shape[-2], ref_images.shape[-1]), dict(legacy=bool(opt.nerf.legacy_coord),
                                                                             depth_inverse=(opt.nerf.depth.param == "inverse"))

    @staticmethod
    def _box_filter(out, h, w, k):
        """The k x k supersampled rows of a (h, w) frame, per output [B, k h k w, C] -> [B, h w, C] (``hip.box_downsample``)."""
        return edict({key: torch.stack([hip.box_downsample(v[b], h, w, k).reshape(h * w, v.shape[-1]) for b in range(v.shape[0])], 0)
                      for key, v in out.items()})

    def _tgt_host(self, tgt_pose):
        """(extrinsics, intrinsics, near_fars) of the target pose on the host; poses generated on the host
        (video paths) carry their numpy originals under "_host" and cost no device sync."""
        if "_host" in tgt_pose:
            return tgt_pose["_host"]
        return tuple(self._host(tgt_pose[k]) for k in ("extrinsics", "intrinsics", "near_fars"))

    # ------------------------------------------------------------------ render (matchnerf.py:88-143)
    def render(self, opt, tgt_pose=None, ray_idx=None, mode=None, ref_poses=None, ref_images=None,
               ref_feats_list=None, ray_range=None, tgt_hw=None, ssaa=1):
        """Rays of one target pose -> edict(rgb [B,N,3], depth [B,N,1], opacity [B,N,1]).
        ``ray_idx`` (LongTensor [N], shared by the batch) selects pixels; ``ray_range`` = (first pixel, count) a contiguous run of
        pixels (a band of rows: dist.render_frame_sharded) that keeps the kernels of the full-frame path; neither = full image.
        ``tgt_hw`` = (h, w): the pixel grid of the target (default: the source views'); ``tgt_pose``'s intrinsics, ``ray_idx`` and
        ``ray_range`` belong to it.  ``ssaa`` = k > 1: k x k rays per pixel (the frame at (k h, k w), intrinsics resized once more),
        box-filtered on the device (``hip.box_downsample``) - full frames and runs of whole rows."""
        if tgt_pose is None:
            raise Exception("Must provide tgt_pose.")
        if not ref_images.is_cuda:
            raise RuntimeError("MatchNeRF.render: the HIP render path needs CUDA tensors (no CPU fallback)")
        batch_size, _, _, img_h, img_w = ref_images.shape
        tgt_h, tgt_w = (img_h, img_w) if tgt_hw is None else (int(tgt_hw[0]), int(tgt_hw[1]))
        device = ref_images.device
        size, ray_kw = self._ray_opts(opt, ref_images)
        n_samples, legacy = size[0], ray_kw["legacy"]
        assert ray_idx is None or ray_range is None
        if int(ssaa) > 1:
            return self._render_ssaa(opt, tgt_pose, int(ssaa), (tgt_h, tgt_w), ray_idx, ray_range, mode, ref_poses, ref_images,
                                     ref_feats_list)
        pix0, n_rays = (0, tgt_h * tgt_w) if ray_range is None else (int(ray_range[0]), int(ray_range[1]))
        if ray_idx is not None:
            n_rays = int(ray_idx.numel())
        idx32 = None if ray_idx is None else ray_idx.to(device=device, dtype=torch.int32).contiguous()
        stratified = mode == "train" and bool(opt.nerf.sample_stratified)

        needs_grad = self._needs_grad(ref_feats_list)
        src = self._sources(ref_poses, ref_images, ref_feats_list)
        tgt_ex, tgt_in, tgt_nf = self._tgt_host(tgt_pose)
        if (needs_grad or mode == "train") and (tgt_h, tgt_w) != (img_h, img_w):
            raise NotImplementedError(f"a target grid {(tgt_h, tgt_w)} other than the views' {(img_h, img_w)} is inference only "
                                      "(the backward kernels answer MNERF_E_UNSUPPORTED)")
        if needs_grad:
            if ray_range is not None:
                ray_idx = torch.arange(pix0, pix0 + n_rays, device=device)
            return self._render_with_grad(opt, src, (tgt_ex, tgt_in, tgt_nf), ray_idx, stratified, ref_images, ref_feats_list, n_rays)
        dec = self._decoder(n_samples, device)
        # [rays*S, cond_stride] hand-off buffer of the staged form: sized for the largest chunk, requested by the first chunk that
        # needs it
        ws_floats = hip.render_workspace_bytes(min(n_rays, MAX_RAYS_PER_LAUNCH), n_samples, dec.cond_stride) // 4
        consts = [camera.target_ray_consts(tgt_ex[b], tgt_in[b], legacy) for b in range(batch_size)]
        strats = [torch.rand(n_rays, n_samples, device=device) for _ in range(batch_size)] if stratified else None

        def launch(b, c, m, *outs):
            # contiguous pixel runs take the matrix form of the cost volume (MNERF_CV_MM=0 keeps the walk); a ray_idx list walks
            sc = src.scene(b, matrix_form=self.cv_matrix_form and idx32 is None)
            rays = hip.make_rays(m, *size, *consts[b], tgt_nf[b, 0], tgt_nf[b, 1], ray_begin=pix0 + c,
                                 ray_idx_ptr=None if idx32 is None else idx32[c:].data_ptr(),
                                 strat_u_ptr=None if strats is None else strats[b][c:].data_ptr(), tgt_hw=(tgt_h, tgt_w), **ray_kw)
            fused = self.fused_render and hip.render_is_fused(sc, dec, rays)
            hip.render_chunk(sc, dec, rays, None if fused else self._workspace(ws_floats, device), *outs,
                             timer=self.kernel_timer, fused=fused)

        return launch_chunks(batch_size, n_rays, MAX_RAYS_PER_LAUNCH, device, launch)

    def _render_ssaa(self, opt, tgt_pose, k, tgt_hw, ray_idx, ray_range, mode, ref_poses, ref_images, ref_feats_list):
        """``render`` with k x k rays per pixel: rows [r0, r1) of the (h, w) frame are rows [k r0, k r1) of the (k h, k w) frame of the
        same camera, rendered as one run of pixels and reduced per output by the box filter on the device, before anything is
        copied or gathered."""
        h, w = tgt_hw
        if ray_idx is not None:
            raise ValueError("render: ssaa > 1 renders full frames or runs of whole rows (ray_range), not a ray_idx list")
        pix0, n = (0, h * w) if ray_range is None else (int(ray_range[0]), int(ray_range[1]))
        if pix0 % w or n % w:
            raise ValueError(f"render: ssaa > 1 needs a ray_range of whole rows, got ({pix0}, {n}) at width {w}")
        hi = self.render(opt, self.resize_pose(tgt_pose, (h, w), (k * h, k * w), bool(opt.nerf.legacy_coord)), mode=mode,
                         ref_poses=ref_poses, ref_images=ref_images, ref_feats_list=ref_feats_list,
                         ray_range=(k * k * pix0, k * k * n), tgt_hw=(k * h, k * w))
        return self._box_filter(hi, n // w, w, k)

    # ------------------------------------------------------------------ caller-supplied rays (include/mnerf.h)
    def render_rays(self, opt, ray_o, ray_d, near_far, mode=None, ref_poses=None, ref_images=None, ref_feats_list=None):
        """Arbitrary rays -> edict(rgb [B,N,3], depth [B,N,1], opacity [B,N,1]).  ``ray_o`` / ``ray_d``: world origins and
        un-normalised world directions, [B,N,3] or [N,3] (shared by the batch), on the device; ``near_far`` [B,2] (or [2]): the
        range of the sample parameter t along o + t d (with unit directions t, and the returned depth, are Euclidean distances).
        Chunks of MAX_RAYS_PER_LAUNCH through one workspace (mnerf_render_rays); results do not depend on the chunking.  Honours
        ``nerf_setbg_opaque``.  Inference only."""
        batch_size = ref_images.shape[0]
        self._inference_only(mode, ref_feats_list, "render_rays")
        if not ref_images.is_cuda:
            raise RuntimeError("MatchNeRF.render_rays: the HIP render path needs CUDA tensors (no CPU fallback)")
        device = ref_images.device
        ray_o, ray_d = (torch.as_tensor(t, dtype=torch.float32, device=device) for t in (ray_o, ray_d))
        if ray_o.shape != ray_d.shape or ray_o.shape[-1] != 3 or ray_o.dim() not in (2, 3):
            raise ValueError(f"render_rays: ray_o {tuple(ray_o.shape)} / ray_d {tuple(ray_d.shape)}: both [B,N,3] or [N,3]")
        if ray_o.dim() == 3 and ray_o.shape[0] != batch_size:
            raise ValueError(f"render_rays: {ray_o.shape[0]} ray sets for a batch of {batch_size}")
        if ray_o.dim() == 2:
            shared = camera.ray_bundle(ray_o, ray_d)
            bundles = [shared] * batch_size
        else:
            bundles = [camera.ray_bundle(ray_o[b], ray_d[b]) for b in range(batch_size)]
        nf = np.broadcast_to(self._host(torch.as_tensor(near_far)).reshape(-1, 2), (batch_size, 2))
        return self._render_bundles(opt, bundles, nf, ref_poses, ref_images, ref_feats_list)

    def _inference_only(self, mode, ref_feats_list, who):
        if self._needs_grad(ref_feats_list) or mode == "train":  # (before the first launch)
            raise NotImplementedError(f"{who}: caller-supplied rays are inference only (no backward kernels over a ray bundle); "
                                      "call it under torch.no_grad() and outside mode='train'")

    def _render_bundles(self, opt, bundles, near_far_host, ref_poses, ref_images, ref_feats_list):
        """``bundles``: per batch element a ray bundle [N, 8] on the device -> edict(rgb, depth, opacity).  Bundles stay on the
        segment walk of the cost volume."""
        device = ref_images.device
        size, ray_kw = self._ray_opts(opt, ref_images)
        n_rays = int(bundles[0].shape[0])
        src = self._sources(ref_poses, ref_images, ref_feats_list)
        dec = self._decoder(size[0], device)
        ws_floats = hip.render_rays_workspace_bytes(min(n_rays, MAX_RAYS_PER_LAUNCH), size[0], dec.cond_stride) // 4

        def launch(b, c, m, *outs):
            rays = hip.make_free_rays(m, *size, near_far_host[b, 0], near_far_host[b, 1], **ray_kw)
            hip.render_rays(src.scene(b), dec, rays, bundles[b][c:c + m], self._workspace(ws_floats, device), *outs)

        return launch_chunks(ref_images.shape[0], n_rays, MAX_RAYS_PER_LAUNCH, device, launch)

    def render_camera(self, opt, tgt_pose, tgt_camera, tgt_hw, ssaa=1, mode=None, ref_poses=None, ref_images=None,
                      ref_feats_list=None):
        """A full (h, w) frame of a target CAMERA MODEL (``target_camera``) at ``tgt_pose``: the camera fills a ray bundle on the
        device (``hip.camera_rays``), the bundle is rendered as caller-supplied rays.  ``ssaa`` = k > 1: the bundle of the same
        camera on the (k h, k w) grid, box-filtered on the device."""
        self._inference_only(mode, ref_feats_list, "render_camera")
        h, w = int(tgt_hw[0]), int(tgt_hw[1])
        k = int(ssaa)
        legacy = bool(opt.nerf.legacy_coord)
        batch_size = ref_images.shape[0]
        tgt_ex, tgt_in, tgt_nf = self._tgt_host(self.resize_pose(tgt_pose, (h, w), (k * h, k * w), legacy))
        args = {key: tgt_camera.get(key) for key in ("fov_deg", "ortho_width", "lon_lat")}
        bundles = [hip.camera_rays(camera.camera_model(tgt_camera["model"], k * h, k * w, tgt_ex[b], tgt_in[b], legacy, **args),
                                   device=ref_images.device) for b in range(batch_size)]
        out = self._render_bundles(opt, bundles, np.asarray(tgt_nf).reshape(batch_size, 2), ref_poses, ref_images, ref_feats_list)
        return out if k == 1 else self._box_filter(out, h, w, k)

    # ------------------------------------------------------------------ geometry export (matchnerf_amd/fusion.py)
    def export_points(self, batch, views="sources", render_path_mode="interpolate", return_maps=False, **fuse_args):
        """The scene of ``batch`` as coloured point clouds -> a list over the batch of [M, 8] float32 device tensors, rows
        ``x y z d | r g b n`` (``fusion.fuse``: depth maps rendered at several poses, kept where other poses confirm them).
        ONE encoder pass; then ``render`` at each fusion pose, depth, opacity and colour staying on the device:
          "sources"   the source views' own poses, at the views' size
          "path"      the poses of the video path (``render_path_mode``, nerf.video_n_frames), on the target grid
          [pose, ..]  dicts of extrinsics [B,3,4] / intrinsics [B,3,3] / near_fars [B,2], on the target grid
        (the target grid: ``batch.tgt_hw`` / nerf.render_hw as in ``forward``; frames are not supersampled).  ``fuse_args``: px_tol,
        rel_tol, min_opacity, min_consistent.  ``return_maps``: -> (clouds, edict(depth [B,K,h,w], opacity [B,K,h,w], rgb [B,K,h*w,3],
        views [[hip.View] * K] * B, hw, counts [[rows of view k] * K] * B)).  The fusion geometry is pinhole z-depth: depth.param =
        inverse and another target camera model are refused, and so are gradients - all before the first launch."""
        from . import fusion
        unknown = set(fuse_args) - {"px_tol", "rel_tol", "min_opacity", "min_consistent"}
        maps, cams_of = self._fusion_maps("export_points", batch, views, render_path_mode, unknown)
        legacy = bool(self.opts.nerf.legacy_coord)
        clouds, all_counts = [], []
        for b, cams in enumerate(cams_of):
            cloud, rows = fusion.fuse(cams, maps.depth[b], maps.opacity[b], maps.rgb[b], maps.hw, legacy, return_counts=True, **fuse_args)
            clouds.append(cloud), all_counts.append(rows)
        if return_maps:
            return clouds, edict(depth=maps.depth, opacity=maps.opacity, rgb=maps.rgb, views=cams_of, hw=maps.hw, counts=all_counts)
        return clouds

    MESH_ARGS = ("bounds", "resolution", "voxel", "trunc", "min_weight", "consistency", "min_component", "min_component_fraction", "smooth",
                 "smooth_lambda", "smooth_mu", "decimate", "sparse")

    @staticmethod
    def check_texture(who, block, power, source, views):
        """the refusals of a texture request, before anything is rendered -> (block, power)"""
        from . import fusion
        block, power = fusion._texture_block(who, block, power)
        if source not in ("render", "images"):
            raise ValueError(f"{who}: texture_from={source!r}: 'render' or 'images'")
        if block and source == "images" and not (isinstance(views, str) and views == "sources"):
            raise ValueError(f"{who}: texture_from='images' bakes the source photographs, so it needs views='sources', not {views!r}")
        return block, power

    def source_colours(self, batch):
        """the source photographs as the colours of the 'sources' fusion views -> [B, K, h*w, 3] float32"""
        images = batch.images[:, :self.n_src_views]
        b, k = images.shape[:2]
        return images.permute(0, 1, 3, 4, 2).reshape(b, k, -1, 3).float().contiguous()

    def export_mesh(self, batch, views="sources", render_path_mode="interpolate", normals=False, texture=0, texture_best=False,
                    texture_power=2, texture_vis_rel_tol=0.02, texture_from="render", texture_visibility="views", report=False, **mesh_args):
        """The scene of ``batch`` as coloured triangle meshes -> a list over the batch of (vertices [V, 8] float32 rows
        ``x y z w | r g b 0``, faces [T, 3] int32) on the device (``fusion.mesh``: the depth maps of ``export_points`` fused into a
        truncated-signed-distance volume, its zero surface extracted by marching tetrahedra).  ``views`` and the one encoder pass as
        in ``export_points``; ``mesh_args``: bounds, resolution, voxel, trunc, min_weight, consistency, the clean-up of
        ``fusion.finish`` (min_component, min_component_fraction, smooth, smooth_lambda, smooth_mu), ``decimate`` (the cell of
        ``fusion.decimate`` in voxels, applied last; 0: none), ``sparse`` (True: the brick-sparse volume of ``fusion.mesh(sparse=True)`` -
        the same mesh in another order, for resolutions past the dense grid) and the thresholds of ``export_points``.  ``normals=True``: triples (vertices, faces, normals [V, 4] float32 rows ``nx ny nz a``,
        ``fusion.vertex_normals`` of the finished mesh).  ``texture=B`` (4..64): the tuples grow by (uv [T, 3, 2], atlas [H, W, 4]) at
        the end - the finished mesh textured with blocks of B texels (``fusion.texture``; ``texture_best``, ``texture_power``,
        ``texture_vis_rel_tol``).  ``texture_from``: "render" bakes the frames rendered at the fusion poses, "images" - with
        ``views="sources"`` only - the source photographs ``batch.images`` instead of their re-renderings; the visibility test uses
        the rendered depth either way - or, with ``texture_visibility="mesh"``, the finished mesh's own depth rasterized at the
        fusion poses (``fusion.texture``).  ``report=True``: -> (meshes, [``fusion.mesh_report`` of every mesh against the maps it
        was fused from, shaded with its atlas when it has one]).  The same refusals, and those of a bad block, power, source or
        visibility, before the first launch."""
        from . import fusion
        unknown = set(mesh_args) - {"px_tol", "rel_tol", "min_opacity", "min_consistent"} - set(self.MESH_ARGS)
        fusion._decimate_cell("export_mesh", mesh_args.get("decimate", 0.0))
        fusion._sparse_flag("export_mesh", mesh_args.get("sparse", False))
        texture, texture_power = self.check_texture("export_mesh", texture, texture_power, texture_from, views)
        fusion._visibility("export_mesh", texture_visibility)
        maps, cams_of = self._fusion_maps("export_mesh", batch, views, render_path_mode, unknown)
        legacy = bool(self.opts.nerf.legacy_coord)
        photos = self.source_colours(batch) if texture and texture_from == "images" else None
        meshes = [fusion.mesh(cams, maps.depth[b], maps.opacity[b], maps.rgb[b], maps.hw, legacy, texture=texture, texture_best=texture_best,
                              texture_power=texture_power, texture_vis_rel_tol=texture_vis_rel_tol,
                              texture_rgbs=None if photos is None else photos[b], texture_visibility=texture_visibility, **mesh_args)
                  for b, cams in enumerate(cams_of)]
        reports = None
        if report:
            min_opacity = mesh_args.get("min_opacity", 0.5)
            reports = [fusion.mesh_report(vertices, faces, cams_of[b], maps.depth[b], maps.opacity[b], maps.rgb[b], maps.hw, legacy,
                                          atlas=textured[1] if textured else None, block=texture, min_opacity=min_opacity)
                       for b, (vertices, faces, *textured) in enumerate(meshes)]
        if normals:
            meshes = [(vertices, faces, fusion.vertex_normals(vertices, faces), *textured) for vertices, faces, *textured in meshes]
        return (meshes, reports) if report else meshes

    def _fusion_maps(self, who, batch, views, render_path_mode, unknown):
        """What ``export_points`` and ``export_mesh`` share: the refusals, ONE encoder pass, a render at each fusion pose ->
        (edict(depth [B,K,h,w], opacity [B,K,h,w], rgb [B,K,h*w,3], hw), [[hip.View] * K] * B)."""
        if self.opts.nerf.depth.param != "metric":
            raise ValueError(f"{who}: nerf.depth.param={self.opts.nerf.depth.param!r}; the fusion geometry is metric camera-z depth")
        if self.target_camera(batch, "test") is not None:
            raise ValueError(f"{who}: the target camera is not a pinhole; the fusion geometry is pinhole camera-z depth")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError(f"{who} is inference only; call it under torch.no_grad()")
        if unknown:
            raise TypeError(f"{who}: unknown arguments {sorted(unknown)}")
        self._src = None
        ref_images = batch.images[:, :self.n_src_views]
        tgt_pose, ref_poses = self.extract_poses(batch)
        batch_size, _, _, img_h, img_w = ref_images.shape
        if isinstance(views, str) and views == "sources":
            hw = (img_h, img_w)
            poses = [dict(extrinsics=ref_poses["extrinsics"][:, v], intrinsics=ref_poses["intrinsics"][:, v],
                          near_fars=ref_poses["near_fars"][:, v]) for v in range(self.n_src_views)]
        else:
            tgt_pose, hw, _ = self.target_grid(batch, "test", tgt_pose, (img_h, img_w))
            if isinstance(views, str) and views == "path":
                poses = self.get_video_rendering_path(tgt_pose, ref_poses, render_path_mode, self.opts.nerf.video_n_frames, batch)
            elif isinstance(views, str):
                raise ValueError(f"{who}: views={views!r}: 'sources', 'path' or a list of pose dicts")
            else:
                poses = list(views)
        if len(poses) < 2:
            raise ValueError(f"{who}: {len(poses)} fusion pose(s); cross-view consistency needs at least 2")
        ref_feats_list = self.get_img_feat(ref_images, attn_splits_list=self.opts.encoder.attn_splits_list,
                                           cur_n_src_views=self.n_src_views)
        rets = [self.render(self.opts, p, mode="test", ref_poses=ref_poses, ref_images=ref_images, ref_feats_list=ref_feats_list,
                            tgt_hw=hw) for p in poses]
        hosts = [self._tgt_host(p) for p in poses]
        depth = torch.stack([r.depth[..., 0] for r in rets], 1).reshape(batch_size, len(poses), hw[0], hw[1])
        opacity = torch.stack([r.opacity[..., 0] for r in rets], 1).reshape(batch_size, len(poses), hw[0], hw[1])
        rgb = torch.stack([r.rgb for r in rets], 1)
        cams_of = [[hip.make_view(ex[b], it[b], nf[b, 0], nf[b, 1]) for ex, it, nf in hosts] for b in range(batch_size)]
        return edict(depth=depth, opacity=opacity, rgb=rgb, hw=hw), cams_of

    def render_poses(self, opt, poses, ref_poses=None, ref_images=None, ref_feats_list=None, tgt_hw=None):
        """Full frames of SEVERAL target poses of one source set (the video loop of matchnerf.py:42-71) with as many poses per
        launch as fit MAX_RAYS_PER_POSE_LAUNCH rays: the poses' camera constants travel as a table in HBM (mnerf_rays.pose_table,
        include/mnerf.h) instead of by value in the kernel arguments.  A 128 x 160 frame is 20 480 rays = 80 decoder tiles, a
        third of the 256 workgroups the decoder keeps resident; three poses per launch fill them.  Results are bit-identical
        to ``render`` pose by pose (tests/test_model_gpu.py).
        -> edict(rgb [n_poses,B,N,3], depth [n_poses,B,N,1], opacity [n_poses,B,N,1]) on the device, or None when a table does
        not apply (a single frame exceeds half a pose launch, H*W not a multiple of 64, more than 5 source views, sample_intvs >
        128, a non-default decoder form: ``hip.render_takes_pose_table``)."""
        batch_size, _, _, img_h, img_w = ref_images.shape
        device = ref_images.device
        tgt_hw = (img_h, img_w) if tgt_hw is None else (int(tgt_hw[0]), int(tgt_hw[1]))
        n_pix = tgt_hw[0] * tgt_hw[1]  # a pose's frame on the TARGET grid
        per_launch = MAX_RAYS_PER_POSE_LAUNCH // n_pix
        if per_launch < 2 or len(poses) < 2 or not ref_images.is_cuda or self.fused_render:
            return None
        size, ray_kw = self._ray_opts(opt, ref_images)
        n_samples = size[0]
        # the hand-off rows of a launch are rays x S x cond_stride floats (3.2 GB for 262 144 rays at S = 128): never more than
        # a quarter of what the device has free, so that a smaller card renders with fewer poses per launch instead of failing
        if ref_images.is_cuda:
            free, _ = torch.cuda.mem_get_info(device)
            row_bytes = n_pix * n_samples * 4 * hip.MNERF_COND_STRIDE_MAX
            per_launch = max(1, min(per_launch, int(free // 4 // max(row_bytes, 1))))
            if per_launch < 2:
                return None
        src = self._sources(ref_poses, ref_images, ref_feats_list)
        dec = self._decoder(n_samples, device)
        if not all(hip.render_takes_pose_table(src.scene(b), dec, n_samples, n_pix) for b in range(batch_size)):  # (the walk)
            return None
        n_poses = len(poses)
        hosts = [self._tgt_host(p) for p in poses]
        rows = np.zeros((batch_size, n_poses, hip.MNERF_POSE_FLOATS), np.float32)
        for b in range(batch_size):
            rows[b] = hip.pose_table_rows([camera.target_ray_consts(ex[b], it[b], ray_kw["legacy"]) + (nf[b, 0], nf[b, 1])
                                           for ex, it, nf in hosts])
        table = torch.from_numpy(rows).to(device)  # one small copy per video; stream-ordered before the launches
        chunk = per_launch * n_pix
        ws_floats = hip.render_workspace_bytes(min(n_poses * n_pix, chunk), n_samples, dec.cond_stride) // 4

        def launch(b, c, m, *outs):  # "rays" = poses x pixels: the outputs of a launch are [poses of the group] x [pixels]
            rays = hip.make_rays(m, *size, rows[b, 0, :9], rows[b, 0, 9:21], rows[b, 0, 21], rows[b, 0, 22], ray_begin=c,
                                 pose_table_ptr=table[b].data_ptr(), rays_per_pose=n_pix, tgt_hw=tgt_hw, **ray_kw)
            hip.render_chunk(src.scene(b), dec, rays, self._workspace(ws_floats, device), *outs, timer=self.kernel_timer, fused=False)

        out = launch_chunks(batch_size, n_poses * n_pix, chunk, device, launch)
        # [B, n_poses * N, C] -> the pose-major result (the batch dimension sits between pose and pixel there; no copy at B = 1)
        return edict({k: v.view(batch_size, n_poses, n_pix, -1).transpose(0, 1).contiguous() for k, v in out.items()})

    def _render_with_grad(self, opt, src, tgt_host, ray_idx, stratified, ref_images, ref_feats_list, n_rays):
        """Training path (matchnerf_amd/autograd.py): forward through the HIP kernels; backward = HIP kernels end to end for the
        ray chunk (mnerf_composite_backward -> mnerf_decoder_backward -> mnerf_cost_volume_backward).  Rays go through in
        chunks of GRAD_RAYS_PER_CALL so that a full-image call under autograd keeps the decoder backward's workspace (11.2 KB
        per sample) bounded.  Scenes are built (``SourceSet.build``) over the feature tensors autograd hands each node."""
        from . import autograd as ag
        device = ref_images.device
        size, ray_kw = self._ray_opts(opt, ref_images)
        n_samples = size[0]
        tgt_ex, tgt_in, tgt_nf = tgt_host
        batch_size = ref_images.shape[0]
        idx_all = torch.arange(n_rays, device=device) if ray_idx is None else ray_idx.to(device)
        dec_mod = self._dec()
        outs = []
        for b in range(batch_size):
            strat_all = torch.rand(n_rays, n_samples, device=device) if stratified else None
            kinv, c2w = camera.target_ray_consts(tgt_ex[b], tgt_in[b], ray_kw["legacy"])
            parts = []
            for c in range(0, n_rays, GRAD_RAYS_PER_CALL):
                idx = idx_all[c:c + GRAD_RAYS_PER_CALL]
                idx32 = idx.to(torch.int32).contiguous()
                strat = None if strat_all is None else strat_all[c:c + GRAD_RAYS_PER_CALL].contiguous()
                m = int(idx.numel())

                def make_rays(strat=strat, kinv=kinv, c2w=c2w, idx32=idx32, m=m, b=b):
                    r = hip.make_rays(m, *size, kinv, c2w, tgt_nf[b, 0], tgt_nf[b, 1], ray_idx_ptr=idx32.data_ptr(),
                                      strat_u_ptr=None if strat is None else strat.data_ptr(), **ray_kw)
                    return r, (idx32, strat)  # the struct holds raw pointers: keep the tensors alive with it

                launch = ag.RayChunkLaunch(
                    opt, dec_mod, make_scene=lambda feats, b=b: src.build(b, feats),
                    make_rays=make_rays, make_decoder=lambda: self._decoder(n_samples, device),
                    view0_extr=src.host[0][b, 0], kinv=kinv, c2w=c2w, ray_idx=idx, width=size[2], n_views=self.n_src_views,
                    setbg_opaque=bool(self.nerf_setbg_opaque))
                parts.append(ag.render_ray_chunk(launch, [f[b] for f in ref_feats_list]))
            outs.append([torch.cat([p[k] for p in parts], 0) for k in range(3)])
        return edict(rgb=torch.stack([o[0] for o in outs], 0), depth=torch.stack([o[1] for o in outs], 0),
                     opacity=torch.stack([o[2] for o in outs], 0))

    def render_by_slices(self, opt, tgt_pose, mode=None, ref_poses=None, ref_images=None, ref_feats_list=None, tgt_hw=None,
                         ssaa=1):
        """matchnerf.py:145-161.  The reference loops over ``rand_rays_<mode>``-sized slices to
        bound memory; the fused kernels have no such temporaries, so the full image is rendered
        in launches of up to MAX_RAYS_PER_LAUNCH rays (identical results, see module docstring)."""
        assert ref_images is not None, "Must provide the reference images for MatchNeRF."
        return self.render(opt, tgt_pose, ray_idx=None, mode=mode, ref_poses=ref_poses, ref_images=ref_images,
                           ref_feats_list=ref_feats_list, tgt_hw=tgt_hw, ssaa=ssaa)

    # ------------------------------------------------------------------ API-compat helpers
    def sample_depth(self, opt, batch_size, num_rays, near_far, legacy=False, mode="train"):
        """matchnerf.py:163-181 (torch; the kernels evaluate the same expression in-register)."""
        s = opt.nerf.sample_intvs
        dev = near_far.device
        depth_min, depth_max = near_far[:, :1], near_far[:, 1:]
        if mode == "train" and opt.nerf.sample_stratified:
            t = torch.rand(batch_size, num_rays, s, 1, device=dev)
        else:
            t = (0.0 if legacy else 0.5) * torch.ones(batch_size, num_rays, s, 1, device=dev)
        t = t + torch.arange(s, device=dev)[None, None, :, None].float()
        d = t / ((s - 1) if legacy else s) * (depth_max - depth_min).reshape(batch_size, 1, 1, 1) \
            + depth_min.reshape(batch_size, 1, 1, 1)
        return dict(metric=d, inverse=1 / (d + 1e-8))[opt.nerf.depth.param]

    def query_cond_info(self, point_samples, ref_poses, ref_images, ref_feats_list, tgt_pose=None, ray_idx=None):
        """matchnerf.py:209-293 through the K1+K2 kernel.  The kernel rebuilds the sample points
        from the target pose, so ``tgt_pose`` (+ optional ``ray_idx``) replaces ``point_samples``
        (kept in the signature for call compatibility; only its shape is used)."""
        if tgt_pose is None:
            raise NotImplementedError("query_cond_info needs tgt_pose: the HIP kernel regenerates the 3D samples")
        b_n, n_rays, n_samples = point_samples.shape[:3]
        v = ref_images.shape[1]
        device = ref_images.device
        size, ray_kw = self._ray_opts(self.opts, ref_images, n_samples)
        src = self._sources(ref_poses, ref_images, ref_feats_list)
        dc = self._dec().cond_dim
        stride = ((dc + 1 + 7) // 8) * 8
        sum_g = dc - 4 * v
        out = torch.empty(b_n, n_rays * n_samples, stride, device=device)
        idx32 = None if ray_idx is None else ray_idx.to(device=device, dtype=torch.int32).contiguous()
        t_ex, t_in, t_nf = self._tgt_host(tgt_pose)
        for b in range(b_n):
            kinv, c2w = camera.target_ray_consts(t_ex[b], t_in[b], ray_kw["legacy"])
            rays = hip.make_rays(n_rays, *size, kinv, c2w, t_nf[b, 0], t_nf[b, 1],
                                 ray_idx_ptr=None if idx32 is None else idx32.data_ptr(), **ray_kw)
            hip.cost_volume(src.scene(b), rays, stride, out=out[b])
        out = out.reshape(b_n, n_rays, n_samples, stride)
        return dict(feat_info=out[..., :sum_g], color_info=out[..., sum_g:sum_g + 3 * v],
                    mask_info=out[..., sum_g + 3 * v:dc])

    def get_img_feat_view_chunks(self, imgs):
        """``get_img_feat`` in the reference's return format [B,V,(V-1)*128,h,w] per scale."""
        return [pair_major_to_view_chunks(f) for f in self.get_img_feat(imgs, cur_n_src_views=self.n_src_views)]

    # ------------------------------------------------------------------ video paths (matchnerf.py:295-325)
    def get_video_rendering_path(self, tgt_pose, ref_poses, mode, n_frames=30, batch=None):
        from . import video
        device = tgt_pose["extrinsics"].device
        per_batch = []
        for bi, src in enumerate(ref_poses["extrinsics"]):
            if mode == "interpolate":
                sq = torch.eye(4).repeat(src.shape[0], 1, 1)
                sq[:, :3] = src.detach().cpu()
                c2ws = sq.double().inverse()[:, :3].float().numpy()
                path = video.interpolate_render_path(c2ws, n_frames)
            elif mode == "spiral":
                assert batch is not None, "Must provide all c2ws and near_far for getting spiral rendering path."
                c2ws_all = batch["c2ws_all"][bi].detach().cpu().numpy()
                nf = tgt_pose["near_fars"][bi].detach().cpu().numpy().tolist()
                path = video.spiral_render_path(c2ws_all, nf, rads_scale=getattr(self.opts.nerf, "video_rads_scale", 0.1),
                                                n_views=n_frames)
            else:
                raise Exception(f"Unknown video rendering path mode {mode}")
            per_batch.append(torch.tensor(np.asarray(path)).inverse()[:, :3].to(torch.float32))
        paths_host = torch.stack(per_batch, 0)                       # [B, n_frames, 3, 4] on the host
        paths = paths_host.to(device)
        _, t_in, t_nf = self._tgt_host(tgt_pose)                     # one device->host copy for the whole path
        paths_np = paths_host.numpy()
        # the reference indexes frames 0..n_frames-1 of the path (matchnerf.py:319-323); "_host" carries the numpy
        # originals so that render() needs no device->host copy per frame
        return [dict(extrinsics=paths[:, i], intrinsics=tgt_pose["intrinsics"].clone().detach(),
                     near_fars=tgt_pose["near_fars"].clone().detach(), _host=(paths_np[:, i], t_in, t_nf))
                for i in range(n_frames)]
