"""Conditions on the inputs of the compositing tests (composite_helpers.py); no kernel runs here.

The GPU tests judge every compositing kernel against float64 at the gates of test_composite_matches_oracle.  Those gates only mean
something where plain float32 arithmetic can meet them with room to spare, and a profile only tests its regime if the draws are in
it.  Both are checked here on the float32 oracle, which a machine without a GPU can run.
"""
import pytest
import torch

import composite_helpers as CH
from oracle import matchnerf_oracle as O


def _oracle32(inp, sigma, wo_interval, setbg, rgb_s=None):
    cfg = O.OracleConfig(wo_render_interval=wo_interval)
    return O.composite(cfg, inp["ray"], inp["rgb_s"] if rgb_s is None else rgb_s, sigma, inp["depth"], setbg_opaque=setbg)


@pytest.mark.parametrize("S", CH.SAMPLE_COUNTS)
def test_float32_oracle_stays_inside_half_the_forward_gates(S):
    """O.composite on float32 tensors vs float64, every profile x interval mode x background: finite everywhere and within half of
    each forward gate (rgb, opacity, prob 2e-6, depth 1e-5)."""
    inp = CH.case_inputs(S)
    worst = {}
    for name, sigma in inp["sigma"].items():
        for wo_interval, setbg in CH.MODES:
            out = _oracle32(inp, sigma, wo_interval, setbg)
            assert all(o.dtype == torch.float32 for o in out)
            ref = CH.composite64(inp["rgb_s"], sigma, inp["depth"], inp["ray"].double().norm(dim=-1), wo_interval, setbg)
            err = CH.forward_errors(out, ref)
            CH.check_forward(err, f"S={S} {name} wo_interval={wo_interval} setbg={setbg}", fraction=0.5)
            for k, e in err.items():
                worst[k] = max(worst.get(k, 0.0), e)
    print(f"\nS={S} float32 oracle vs float64, worst over profiles and modes: " + ", ".join(f"{k} {e:.2e}" for k, e in worst.items()))


@pytest.mark.parametrize("S", CH.BACKWARD_SAMPLE_COUNTS)
def test_float32_oracle_gradients_stay_inside_half_the_backward_gates(S):
    """float32 autograd through O.composite vs float64 autograd, all columns, density gradient normalised by k_j: within half of
    2e-6 max(1, max|ref|) (colours) and 2e-5 max(1, max|ref|) (density)."""
    inp = CH.case_inputs(S)
    worst = [0.0, 0.0]
    for name, sigma in inp["sigma"].items():
        for wo_interval, setbg in CH.MODES:
            rgb_s = inp["rgb_s"].clone().requires_grad_(True)
            sig = sigma.clone().requires_grad_(True)
            out = _oracle32(inp, sig, wo_interval, setbg, rgb_s)
            ((out[0] * inp["g_rgb"]).sum() + (out[1][:, 0] * inp["g_depth"]).sum() + (out[2][:, 0] * inp["g_opacity"]).sum()).backward()
            ref = CH.gradients64(inp, sigma, wo_interval, setbg)
            e_rgb, gate_rgb, e_sd, gate_sd = CH.backward_errors(rgb_s.grad, sig.grad, ref)
            what = f"S={S} {name} wo_interval={wo_interval} setbg={setbg}"
            assert e_rgb < 0.5 * gate_rgb, f"{what}: g_rgb_s error {e_rgb:.2e} >= {0.5 * gate_rgb:.1e}"
            assert e_sd < 0.5 * gate_sd, f"{what}: dL/dsd error {e_sd:.2e} >= {0.5 * gate_sd:.1e}"
            worst = [max(worst[0], e_rgb / gate_rgb), max(worst[1], e_sd / gate_sd)]
    print(f"\nS={S} float32 autograd vs float64, worst error / gate: g_rgb_s {worst[0]:.2f}, dL/dsd {worst[1]:.2f}")


@pytest.mark.parametrize("S", CH.SAMPLE_COUNTS)
def test_profiles_are_in_the_regime_they_name(S):
    """Without intervals (sd = sigma, so the profile's numbers are the optical depths):
    wall and wall_first have rays with opacity > 1 - 1e-6; wall and block_edge have samples whose float32 transmittance is exactly
    0, and so do wall_first and slab at the values the exact-zero tests use (200); at their parity values (50 and five times 3.0)
    the transmittance behind them is below 1e-6 and 1e-6 respectively but not 0, which is asserted as such; zero gives opacity
    exactly 0; tiny gives opacity exactly 0 in float32 (1 - exp(-1e-30) rounds to 0)."""
    inp = CH.case_inputs(S)
    sig = inp["sigma"]
    assert list(sig)[:8] == ["fog", "wall", "wall_first", "wall_last", "slab", "all_huge", "zero", "tiny"]
    assert ("block_edge" in sig) == (S > 64)
    for name, s in sig.items():
        assert s.dtype == torch.float32 and s.shape == (CH.N_RAYS, S) and bool(torch.isfinite(s).all()) and bool((s >= 0).all())
    opacity = {n: _oracle32(inp, s, True, False)[2][:, 0] for n, s in sig.items()}
    prefix = {n: CH.prefix64(s, inp["depth"], inp["ray_len"], True) for n, s in sig.items()}
    t32 = {n: torch.exp(-torch.cat([torch.zeros(CH.N_RAYS, 1), s[:, :-1]], 1).cumsum(1)) for n, s in sig.items()}
    for name in ("wall", "wall_first"):
        assert int((opacity[name] > 1 - 1e-6).sum()) > 0, name
    assert bool((opacity["wall_first"] > 1 - 1e-6).all())
    assert float(opacity["zero"].abs().max()) == 0.0 and float(opacity["tiny"].abs().max()) == 0.0
    if S > 1:
        for name in ("wall",) + (("block_edge",) if S > 65 else ()):  # at S = 65 block_edge's wall is the last sample
            zero = prefix[name] > CH.T_ZERO
            assert int(zero.sum()) > 0 and float(t32[name][zero].abs().max()) == 0.0, name
        assert float(t32["wall_first"][:, 1:].max()) < 1e-6 and float(t32["wall_first"].min()) > 0.0
        strong = CH.case_inputs(S, wall_first_value=200.0, slab_value=200.0)["sigma"]
        for name in ("wall_first", "slab") if S > 5 else ("wall_first",):
            p = CH.prefix64(strong[name], inp["depth"], inp["ray_len"], True)
            zero = p > CH.T_ZERO
            assert int(zero.sum()) > 0, name
            t = torch.exp(-torch.cat([torch.zeros(CH.N_RAYS, 1), strong[name][:, :-1]], 1).cumsum(1))
            assert float(t[zero].abs().max()) == 0.0, name
    if S > 5:  # behind a whole slab of 5 x 3.0 the transmittance is exp(-15) = 3e-7
        behind = prefix["slab"] >= 15.0
        assert int(behind.sum()) > 0 and float(t32["slab"][behind].max()) < 1e-6
    if S > 64:
        assert bool((sig["block_edge"][:, 63] == 0.7).all()) and bool((sig["block_edge"][:, 64] == 200.0).all())
    # with intervals the last sample's interval is 1e10: any ray whose last density is positive is opaque
    assert bool((_oracle32(inp, sig["wall_last"], False, False)[2][:, 0] > 1 - 1e-6).all())
