"""Sharded evaluation on the GPU: `python test.py --gpu_ids=0,1` against the one-process run, and validation inside a two-rank
`python train.py`.  The GPU box has one MI355X: both ranks share it (MNERF_FORCE_DEVICE=0) and talk through gloo, as in
tests/test_train_dist_gpu.py; every child runs under `timeout -k 10`, nothing is retried, at most two ranks hold the GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu


def _run(script, args, cwd, limit=420):
    env = dict(os.environ, MNERF_FORCE_DEVICE="0", MNERF_DIST_BACKEND="gloo")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "MNERF_DIST_INIT_ALWAYS", "MNERF_DEVICE_METRICS"):
        env.pop(k, None)
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.join(REPO, script)] + args, cwd=cwd, env=env,
                       capture_output=True, text=True)
    print(r.stdout[-3000:], r.stderr[-3000:])
    return r


def test_test_py_with_two_ranks_writes_the_one_process_report(tmp_path):
    """3 synthetic dtu scenes at 48 x 32, S = 16: rank 0 renders batches 0 and 2, rank 1 batch 1; rank 0 alone writes
    0results_dtu.txt, byte for byte the file of the one-process run; with --separate_save every rank writes its own images"""
    args = ["--yaml=test", "--nerf.sample_intvs=16", "--data_test.llff=", "--data_test.blender=", "--data_test.tnt=",
            "--data_test.dtu.img_wh=48,32", "--data_test.dtu.max_len=3", "--separate_save=true", f"--output_root={tmp_path}"]
    one = _run("test.py", args + ["--name=one"], tmp_path)
    assert one.returncode == 0
    two = _run("test.py", args + ["--name=two", "--gpu_ids=0,1"], tmp_path)
    assert two.returncode == 0
    want = open(tmp_path / "one" / "test" / "0results_dtu.txt", "rb").read()
    assert want.count(b"\n") == 4 and want.startswith(b"dtu_000_0: PSNR ")
    found = [os.path.join(d, f) for d, _, fs in os.walk(tmp_path / "two") for f in fs if f.startswith("0results")]
    assert found == [str(tmp_path / "two" / "test" / "0results_dtu.txt")]
    assert open(found[0], "rb").read() == want
    assert two.stdout.count("[coach] dtu: mean PSNR") == 1  # rank 0 alone prints
    assert sorted(os.listdir(tmp_path / "two" / "test")) == ["0results_dtu.txt", "dtu_000_0.png", "dtu_001_0.png", "dtu_002_0.png"]


def test_train_py_with_two_ranks_validates_on_both(tmp_path):
    """two ranks, 4 training scenes = 2 iterations, validation after each (val_it = ceil(0.5 * 2) = 1) over 3 scenes (shares 2 + 1):
    rank 0 alone logs val/PSNR, finite, and every pass leaves its three strips"""
    args = ["--yaml=train", "--name=ddpval", "--gpu_ids=0,1", "--max_epoch=1", "--tb=false", "--data_train.img_wh=64,64",
            "--data_train.max_len=4", "--data_val.img_wh=64,64", "--data_val.max_len=3", "--nerf.rand_rays_train=96",
            "--nerf.rand_rays_val=4096", "--freq.ckpt_ep=-1", "--freq.ckpt_it=-1", "--freq.val_it=0.5", "--freq.val_ep=-1",
            "--freq.test_ep=-1", "--freq.scalar=1", "--data_test.llff=", "--data_test.blender=", "--data_test.dtu.img_wh=64,64",
            "--data_test.dtu.max_len=1", "--nerf.sample_intvs=16", "--nerf.rand_rays_test=4096", f"--output_root={tmp_path}"]
    r = _run("train.py", args, tmp_path)
    assert r.returncode == 0
    out = tmp_path / "ddpval"
    assert "training done: 2 iterations" in r.stdout
    rows = [json.loads(l) for l in open(out / "scalars.jsonl")]
    val = [x for x in rows if x["split"] == "val" and x["tag"] == "PSNR"]
    passes = sorted({x["step"] for x in val})
    assert len(val) == len(passes) >= 1  # one line per pass: rank 0 alone logged
    assert all(np.isfinite(x["value"]) for x in val)
    assert r.stdout.count("[coach] validation at iteration") == len(passes)
    assert all("over 3 images" in l for l in r.stdout.splitlines() if "[coach] validation at iteration" in l)
    strips = sorted(os.listdir(out / "validation"))
    for it in passes:
        assert [s for s in strips if s.endswith(f"_it{it}.jpg")] == [f"synthetic{i}_{i:03d}_0_it{it}.jpg" for i in range(3)]
    assert len(strips) == 3 * len(passes)
