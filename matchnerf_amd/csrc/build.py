"""Build libmnerf_hip.so (gfx950) in-tree:  python -m matchnerf_amd.csrc.build

hipcc cross-compiles without a GPU.  The .so lands next to the package
(matchnerf_amd/libmnerf_hip.so): git-ignored, but it travels to the GPU box with the snapshot.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
OUT = os.path.join(PKG, "libmnerf_hip.so")
SOURCES = ["api.cpp", "backward.hip", "composite.hip", "conv.hip", "conv_backward.hip", "cost_volume.hip", "cost_volume_mm.hip", "decoder.hip", "decoder_backward.hip", "decoder_fused.hip", "encoder_backward.hip", "encoder_block.hip",
           "free_rays.hip", "fusion.hip", "gemm.hip", "geometry.hip", "instance_norm.hip", "lpips.hip", "mesh.hip", "mesh_finish.hip", "mesh_raster.hip", "mesh_texture.hip", "metrics.hip", "optim.hip", "qkv.hip", "render_chunk.hip", "scan.hip", "tsdf_sparse.hip", "window_attention.hip", "window_attention_backward.hip"]
# per-source extra flags.
# decoder_fused.hip: the one-launch ray chunk.  Its workgroups run the cost-volume walk on SIMDs where another workgroup issues
# 16-bit 32x32x16 matrix instructions; packed-fp32 vector instructions lose results in lanes 48-63 there, so
# that object is built without them: the walk's channel-pair arithmetic is one instruction per channel (cv_walk.hpp) and the SLP
# vectoriser is off.
# cost_volume.hip: the same rule for the stand-alone kernel (it may share SIMDs with 16-bit MFMA
# waves of ANY kernel on another stream; measured next to this library's decoder), and the same arithmetic as the walk
# inside the one-launch form, so that the two forms stay bit-identical.
# decoder.hip: the same flag — the two forms of the ray chunk are bit-identical only if their trunks are
# compiled alike, and the trunk's own packed multiplies sat next to the partner workgroup's matrix instructions too;
# measured neutral (19.60 vs 19.75 ms per frame).
EXTRA_FLAGS = {"cost_volume.hip": ["-fno-slp-vectorize"], "cost_volume_mm.hip": ["-fno-slp-vectorize"], "decoder.hip": ["-fno-slp-vectorize"],
               "decoder_fused.hip": ["-fno-slp-vectorize"]}
# what the decoder kernels are compiled from
DECODER_SOURCES = ["decoder.hip", "decoder_fused.hip", "decoder_staged.hpp", "decoder_common.hpp", "split_f16.hpp", "cv_walk.hpp", "common.hpp"]
# -amdgpu-use-amdgpu-trackers: the AMDGPU register-pressure trackers in the scheduler; the fused decoder spills 57 instead
# of 108 vector registers with them (decoder 20.8 -> 20.15 ms per frame on MI355X), everything else is unchanged
# -target-feature -packed-fp32-ops (ALL device code): the compiler may not select v_pk_{mul,fma,add}_f32.  On gfx950 a packed-fp32
# vector instruction that consumes freshly returned VMEM / LDS data can lose its result in lanes 48-63 while another wave of the
# SIMD issues 16-bit 32x32x16 matrix instructions.  Rounds 2-3 removed the packed forms from the walk by
# hand and with -fno-slp-vectorize; the loop vectoriser still produced them in decoder_kernel<8,256,*> (round-3 verdict), and
# every other kernel of the library is a possible victim next to an MFMA kernel on another stream.  With the target feature off
# no object of the library contains one (tests/test_isa.py disassembles the shipped .so); the price is 3-16 % more vector
# instructions in the encoder kernels' operand splits (conv 26.3 k -> 27.1 k static VALU instructions, K7 3.5 k -> 4.0 k).
NO_PACKED_F32 = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "-mllvm",
         "-amdgpu-use-amdgpu-trackers=1"] + NO_PACKED_F32


def _hash(flags_of, sources, structs):
    """sha256 over what a kernel is compiled from: the compiler flags (those of the source `flags_of`), the text of `sources` and
    the argument structs it takes from the ABI header."""
    import hashlib
    import re
    h = hashlib.sha256(" ".join(FLAGS + EXTRA_FLAGS.get(flags_of, [])).encode())
    for name in sorted(sources):
        with open(os.path.join(HERE, name), "rb") as f:
            h.update(name.encode() + b"\0" + f.read())
    with open(os.path.join(PKG, "..", "include", "mnerf.h")) as f:
        header = f.read()
    for st in structs:
        m = re.search(r"typedef struct %s \{.*?\} %s;" % (st, st), header, re.S)
        h.update(m.group(0).encode())
    return h.hexdigest()[:16]


def source_hash():
    """sha256 over everything the decoder kernels are compiled from (their sources, the argument structs they take from the
    ABI header, the compiler flags): identifies the build that profile-derived numbers (profiles/current/decoder_counters.json)
    belong to, so that bench.py can tell when they have gone stale.  (Other kernels' sources and the rest of the header
    are left out: a change in the encoder does not change the decoder's counters.)"""
    return _hash("decoder.hip", DECODER_SOURCES, ("mnerf_view", "mnerf_rays", "mnerf_scene", "mnerf_decoder"))


COST_VOLUME_SOURCES = ["cost_volume.hip", "cost_volume_mm.hip", "cv_walk.hpp", "common.hpp"]  # what cost_volume_lean_kernel is compiled from


def cost_volume_source_hash():
    """The same for the stand-alone cost-volume kernel (profiles/current/cost_volume_counters.json)."""
    return _hash("cost_volume.hip", COST_VOLUME_SOURCES, ("mnerf_view", "mnerf_rays", "mnerf_scene"))


def _compile(cmd):
    """Run one hipcc compile.  The x86 host pass of a .hip file prints "'-packed-fp32-ops' is not a recognized feature for this
    target (ignoring feature)" for NO_PACKED_F32 (clang has no device-only spelling for -Xclang options; the gfx950 pass honours
    it: tests/test_isa.py): that one line is dropped, everything else the compiler says is passed through."""
    r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
    noise = "'-packed-fp32-ops' is not a recognized feature for this target"
    err = "".join(l for l in r.stderr.splitlines(True) if noise not in l)
    if err:
        sys.stderr.write(err)
    if r.returncode != 0:
        raise subprocess.CalledProcessError(r.returncode, cmd)


def _newer(a, b):
    return (not os.path.exists(b)) or os.path.getmtime(a) > os.path.getmtime(b)


def build(force=False, verbose=True):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = "hipcc"
    objdir = os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    deps = [os.path.join(HERE, h) for h in sorted(os.listdir(HERE)) if h.endswith(".hpp")] + [os.path.join(PKG, "..", "include", "mnerf.h")]
    objs = []
    for src in SOURCES:
        name = os.path.splitext(src)[0]
        extra = EXTRA_FLAGS.get(src, [])
        sp = os.path.join(HERE, src)
        if not os.path.exists(sp):
            raise FileNotFoundError(sp)
        obj = os.path.join(objdir, name + ".o")
        cmd = [hipcc] + FLAGS + extra + (["-x", "hip"] if src.endswith(".cpp") else []) + ["-c", sp, "-o", obj]
        stamp = obj + ".cmd"  # the command line an object was built with: a change of flags rebuilds it
        same_cmd = os.path.exists(stamp) and open(stamp).read() == " ".join(cmd)
        if force or not same_cmd or _newer(sp, obj) or any(_newer(d, obj) for d in deps):
            if verbose:
                print("[build]", " ".join(cmd), flush=True)
            _compile(cmd)
            with open(stamp, "w") as f:
                f.write(" ".join(cmd))
        objs.append(obj)
    if force or any(_newer(o, OUT) for o in objs):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", OUT] + objs
        if verbose:
            print("[build]", " ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return OUT


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print(OUT)
