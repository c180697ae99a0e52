"""Every packed weight stream keeps its bytes: sha256(bytes)[:16] of each stream against a value recorded from the packers as
they were before the layout code moved into matchnerf_amd/wstream.py.  The twin tests (test_packing_cpu.py) compare the host and
device packers with each other, and both now evaluate the same description; this file pins the description itself.

The inputs use no RNG and no libm: integer arithmetic and one IEEE division."""
import hashlib

import numpy as np
import pytest
import torch

from matchnerf_amd import cond_nerf as CN, gmflow, options


def det(shape, seed, scale):
    n = int(np.prod(shape))
    k = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(seed)) % np.uint64(65521)
    return ((k.astype(np.float32) / np.float32(65521) - np.float32(0.5)) * np.float32(scale)).reshape(shape)


def digest(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


# (legacy, views) -> cond dim, cond stride, {packer: (digest, floats)}, digest of the small block (None: not recorded)
DECODER = {
    (True, 3): (22, 24, {"pack_wstream": ("53166ee2cd4fb534", 136960), "pack_wstream16": ("1ea2c0fc652d1790", 206848),
                         "pack_wstream_h": ("d4f99de2cc3dfcc3", 139776)}, "317f2482ff3c1c8d"),
    (False, 5): (30, 32, {"pack_wstream": ("e1fcbad8dc5ac6f1", 137984), "pack_wstream16": ("5c7717f4e9a9f7f1", 206848),
                          "pack_wstream_h": ("7b4fd66309a04ba8", 139776)}, None),
    (True, 7): (38, 40, {"pack_wstream": ("97bf3ece1dff4990", 139008), "pack_wstream16": ("d338a33f5d0d60bc", 209920),
                         "pack_wstream_h": ("50ef99edf6b4340c", 141824)}, "317f2482ff3c1c8d"),  # 3 FiLM K16-steps: an odd count
}


@pytest.mark.parametrize("legacy,n_views", sorted(DECODER))
def test_decoder_streams_keep_their_bytes(legacy, n_views):
    cond_dim, cond_stride, streams, small = DECODER[(legacy, n_views)]
    opt = options.load_options("configs/test.yaml", verbose=False)
    opt.device = "cpu"
    opt.nerf.legacy_coord, opt.n_src_views, opt.decoder.raytrans_posenc = legacy, n_views, False
    dec = CN.CondNeRF(opt)
    with torch.no_grad():
        for i, (_, p) in enumerate(dec.named_parameters()):
            p.copy_(torch.from_numpy(det(tuple(p.shape), 101 + i, 2.0 ** (i % 7 - 4))))
        dec.pts_linears[2].weight.zero_()
    sd = {"nerf_dec." + k: v for k, v in dec.state_dict().items()}
    for name, (want, floats) in streams.items():
        ws, cd, cs = getattr(CN, name)(sd, n_views, list(opt.encoder.cos_n_group), dec.L_3D, legacy)
        assert (cd, cs) == (cond_dim, cond_stride) and ws.dtype == np.float32 and ws.size == floats, name
        assert digest(ws) == want, name
    if small is not None:
        assert digest(CN.pack_small(sd, 64, False)) == small
    ws, _, cs = dec._packed_on_device(64, torch.device("cpu"))
    assert cs == cond_stride and digest(ws) == streams["pack_wstream_h"][0]


CONV = [("pack_conv", (64, 64, 3, 3), 1, 0.1, 36864, 18, "f7b21ecedca225cf"),
        ("pack_conv", (128, 96, 1, 1), 2, 3.0, 12288, 13, "b4f23c6c111b8ed9"),
        ("pack_conv_blocks", (64, 3, 3, 3), 3, 0.5, 18432, 16, "7571e8161795faca"),
        ("pack_conv_blocks", (256, 128, 3, 3), 4, 0.02, 294912, 20, "002142600408bcd8"),
        ("pack_conv_stem", (64, 3, 7, 7), 5, 0.2, 10240, 17, "85f3911587078c7c")]


@pytest.mark.parametrize("name,shape,seed,scale,floats,ew,want", CONV)
def test_conv_streams_keep_their_bytes(name, shape, seed, scale, floats, ew, want):
    ws, e = getattr(gmflow, name)(det(shape, seed, scale))
    assert ws.dtype == np.float32 and ws.size == floats and e == ew
    assert digest(ws) == want


def test_qkv_stream_keeps_its_bytes():
    ws, ews = gmflow.pack_qkv(det((128, 128), 6, 0.09), det((128, 128), 7, 0.4), det((128, 128), 8, 2.0))
    assert ws.dtype == np.float32 and ws.size == 49152 and ews == (18, 16, 13)
    assert digest(ws) == "f58b63effc409037"


@pytest.mark.parametrize("ffn,floats,ews,want", [(False, 16384, (18, 0, 0), "62b51d8e34e9719b"),
                                                 (True, 409600, (18, 19, 20), "fd6573a857e18440")])
def test_encoder_block_stream_keeps_its_bytes(ffn, floats, ews, want):
    w0, w2 = (det((1024, 256), 10, 0.05), det((128, 1024), 11, 0.03)) if ffn else (None, None)
    ws, e = gmflow.pack_encoder_block(det((128, 128), 9, 0.1), w0, w2)
    assert ws.dtype == np.float32 and ws.size == floats and e == ews
    assert digest(ws) == want
