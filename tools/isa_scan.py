"""Disassemble the gfx950 code objects of a built libmnerf_hip.so and report, per kernel, the instructions that matter for
the packed-fp32 / 16-bit-MFMA erratum of DESIGN.md section 4 (and a few register facts).

    python tools/isa_scan.py [path/to/libmnerf_hip.so]          # table on stdout
    python tools/isa_scan.py --digest a.so [b.so]               # per symbol: instruction count + hash; two paths: what differs
    from tools.isa_scan import scan; scan(path) -> {kernel: {...}}

What is counted per kernel (demangled name):
  pk_f32    v_pk_{mul,fma,add}_f32 instructions
  mfma16    16-bit 32x32x16 / 16x16x32 matrix instructions (v_mfma_f32_32x32x16_{f16,bf16}, v_mfma_f32_16x16x32_*)
  mfma      all matrix instructions
  scratch   scratch_{load,store} instructions (register spills)

Works without a GPU (llvm-objdump from the ROCm image).  The library is copied to a temporary directory first:
`llvm-objdump --offloading` writes the extracted bundles next to its input.
"""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM_BIN = "/opt/rocm/lib/llvm/bin"
PK_F32 = re.compile(r"\bv_pk_(mul|fma|add)_f32\b")
MFMA16 = re.compile(r"\bv_mfma_f32_(32x32x16|16x16x32)_(f16|bf16)\b")
MFMA = re.compile(r"\bv_mfma_")
SCRATCH = re.compile(r"\bscratch_(load|store)_")
SYM = re.compile(r"^[0-9a-f]+ <(.+)>:$")


def _tool(name):
    p = os.path.join(LLVM_BIN, name)
    return p if os.path.exists(p) else name


def _disassembly(lib_path):
    """(code object, demangled symbol, line) for every line of every gfx950 code object's disassembly that belongs to a symbol"""
    with tempfile.TemporaryDirectory() as tmp:
        lib = os.path.join(tmp, "lib.so")
        shutil.copy(lib_path, lib)
        subprocess.run([_tool("llvm-objdump"), "--offloading", lib], check=True, stdout=subprocess.DEVNULL,
                       stderr=subprocess.DEVNULL)
        bundles = sorted(f for f in os.listdir(tmp) if "gfx950" in f)
        if not bundles:
            raise RuntimeError(f"no gfx950 code object in {lib_path}")
        for n, b in enumerate(bundles):
            dis = subprocess.run([_tool("llvm-objdump"), "-d", "--demangle", os.path.join(tmp, b)], check=True,
                                 capture_output=True, text=True).stdout
            cur = None
            for line in dis.splitlines():
                m = SYM.match(line)
                if m:
                    cur = m.group(1)
                elif cur is not None:
                    yield n, cur, line


def scan(lib_path):
    """{demangled kernel name: {"pk_f32": n, "mfma16": n, "mfma": n, "scratch": n, "pk_lines": [first few]}}"""
    out = {}
    for _, cur, line in _disassembly(lib_path):
        rec = out.setdefault(cur, {"pk_f32": 0, "mfma16": 0, "mfma": 0, "scratch": 0, "pk_lines": []})
        if PK_F32.search(line):
            rec["pk_f32"] += 1
            if len(rec["pk_lines"]) < 4:
                rec["pk_lines"].append(line.strip().split("//")[0].strip())
        if MFMA.search(line):
            rec["mfma"] += 1
            if MFMA16.search(line):
                rec["mfma16"] += 1
        if SCRATCH.search(line):
            rec["scratch"] += 1
    return out


def digest(lib_path):
    """{demangled symbol: (instructions, sha256 of the normalised instruction text)}; a template instance that several objects
    hold is listed once per object ("name #2", in the order of the code objects).  Normalised: no addresses or encodings, nothing
    behind the last s_endpgm (padding), and the literal of the s_add_u32 / s_addc_u32 behind an s_getpc_b64 masked: a pc-relative
    address of a table in the code object, which moves when the symbol's neighbours in the object change."""
    text, copies = {}, {}
    for n, cur, line in _disassembly(lib_path):
        ins = " ".join(line.split("//")[0].split())
        if not ins:
            continue
        objs = copies.setdefault(cur, [])
        if n not in objs:
            objs.append(n)
        t = text.setdefault(cur if objs.index(n) == 0 else f"{cur} #{objs.index(n) + 1}", [])
        if any(p.startswith("s_getpc_b64") for p in t[-2:]) and re.match(r"s_addc?_u32 ", ins):
            ins = ins.rsplit(" ", 1)[0] + " <pc-relative>"
        t.append(ins)
    out = {}
    for k, t in text.items():
        ends = [i for i, x in enumerate(t) if x.startswith("s_endpgm")]
        t = t[: ends[-1] + 1] if ends else t
        out[k] = (len(t), hashlib.sha256("\n".join(t).encode()).hexdigest()[:16])
    return out


def short(name, n=86):
    name = re.sub(r"\(.*$", "", name)  # drop the argument list
    return name if len(name) <= n else name[: n - 3] + "..."


if __name__ == "__main__" and "--digest" in sys.argv:
    paths = [a for a in sys.argv[1:] if a != "--digest"]
    d = [digest(p) for p in paths]
    if len(d) == 1:
        for k in sorted(d[0]):
            print(f"{d[0][k][0]:7d} {d[0][k][1]} {k}")
    else:
        a, b = d
        for k in sorted(set(a) | set(b)):
            if a.get(k) != b.get(k):
                print(f"DIFFERS {a.get(k, 'absent')} -> {b.get(k, 'absent')} {k}")
        same = sum(1 for k in a if a[k] == b.get(k))
        print(f"{same} of {len(set(a) | set(b))} symbols identical ({len(a)} in {paths[0]}, {len(b)} in {paths[1]})")
        sys.exit(0 if same == len(set(a) | set(b)) else 1)
elif __name__ == "__main__":
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(here, "matchnerf_amd", "libmnerf_hip.so")
    res = scan(path)
    print(f"{'kernel':86s} {'pk_f32':>6s} {'mfma16':>6s} {'mfma':>6s} {'scratch':>7s}")
    for k in sorted(res):
        r = res[k]
        print(f"{short(k):86s} {r['pk_f32']:6d} {r['mfma16']:6d} {r['mfma']:6d} {r['scratch']:7d}")
