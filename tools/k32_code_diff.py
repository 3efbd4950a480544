"""Development check: the gfx950 code of every kernel instantiation that exists in a base revision (default HEAD) is unchanged
in the working tree -- for knn.hip and vecattn.hip by default.  Both versions' sources are compiled device-only, disassembled,
and compared kernel by kernel (encodings, addresses and the PC-relative offsets of globals, which move with the code size,
are left out; the alignment padding after the last s_endpgm too).  Kernels new in the working tree are listed, not compared.

  python tools/k32_code_diff.py [--base REV] [file.hip ...]      exit 1 when a pre-existing kernel changed
  python tools/k32_code_diff.py --base <parent commit> attn.hip gemm.hip knn.hip vecattn.hip      the N_SAMPLE change: the masked attention kernels are new
                                                                            names (attn_kernels.inc compiled twice), nothing else moves"""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "poem-v2_amd/csrc"
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", "--cuda-device-only",
         "--no-gpu-bundle-output", "-c"]


def disassemble(src_dir, name, tmp):
    obj = os.path.join(tmp, name + ".co")
    subprocess.run([os.path.join(ROCM, "bin", "hipcc"), *FLAGS, os.path.join(src_dir, name), "-o", obj], check=True,
                   stderr=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(ROCM, "llvm", "bin", "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", obj],
                         check=True, capture_output=True, text=True).stdout
    funcs, cur, prev = {}, None, ""
    for line in out.splitlines():
        m = re.match(r"^<(\S+)>:$", line.strip())
        if m:
            cur = m.group(1)
            funcs[cur] = []
            continue
        ins = re.sub(r"\s+", " ", line.split("//")[0].strip())
        if prev.startswith("s_getpc_b64") and ins.startswith("s_add_u32"):
            ins = re.sub(r"0x[0-9a-f]+$", "<pcrel>", ins)
        if cur and ins and ins != "...":
            funcs[cur].append(ins)
            prev = ins
    for k, body in funcs.items():       # inter-function padding (zero words) decodes as instructions after the last s_endpgm
        while body and body[-1] != "s_endpgm":
            body.pop()
    return funcs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", default="HEAD")
    ap.add_argument("files", nargs="*", default=["knn.hip", "vecattn.hip"])
    a = ap.parse_args()
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        base_dir = os.path.join(tmp, "base")
        os.makedirs(base_dir)
        tar = subprocess.run(["git", "-C", ROOT, "archive", a.base, CSRC], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", base_dir], input=tar, check=True)
        for f in a.files:
            old = disassemble(os.path.join(base_dir, CSRC), f, tmp)
            new = disassemble(os.path.join(ROOT, CSRC), f, tmp)
            for k, body in old.items():
                if k not in new:
                    print(f"{f}: MISSING {k}")
                    bad += 1
                elif body != new[k]:
                    print(f"{f}: CHANGED {k}")
                    print("\n".join(list(difflib.unified_diff(body, new[k], lineterm="", n=1))[:20]))
                    bad += 1
            print(f"{f}: {len(old)} kernels of {a.base} compared, new: {sorted(set(new) - set(old))}")
    print("identical" if not bad else f"{bad} kernel(s) differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
