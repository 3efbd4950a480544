"""Development check: the gfx950 code of every kernel instantiation that exists in a base revision (default HEAD) is unchanged
in the working tree -- for every .hip file of csrc/ (either version's) unless files are named.  Both versions' sources are
compiled device-only, disassembled, and compared kernel by kernel (encodings, addresses and the PC-relative offsets of globals,
which move with the code size, are left out; the alignment padding after the last s_endpgm too).  Kernels new in the working
tree are listed, not compared.

  python tools/k32_code_diff.py [--base REV] [file.hip ...]      exit 1 when a pre-existing kernel changed
  python tools/k32_code_diff.py --base <parent commit>           a refactor: "identical", and `new: []` on every file's line
  python tools/k32_code_diff.py --base <parent commit> attn.hip gemm.hip knn.hip vecattn.hip      the N_SAMPLE change: the masked attention kernels are new
                                                                            names (attn_kernels.inc compiled twice), nothing else moves"""
import argparse
import concurrent.futures
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "poem-v2_amd/csrc"
INCLUDE = "include"             # csrc's sources include the public header by its relative path
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", "--cuda-device-only",
         "--no-gpu-bundle-output", "-c"]


def disassemble(src_dir, name, tmp):
    if not os.path.exists(os.path.join(src_dir, name)):      # a file only one version has: all its kernels are missing / new
        return {}
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
    ap.add_argument("files", nargs="*")
    a = ap.parse_args()
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        base_dir = os.path.join(tmp, "base")
        os.makedirs(base_dir)
        tar = subprocess.run(["git", "-C", ROOT, "archive", a.base, CSRC, INCLUDE], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", base_dir], input=tar, check=True)
        both = os.listdir(os.path.join(base_dir, CSRC)) + os.listdir(os.path.join(ROOT, CSRC))
        files = a.files or sorted({n for n in both if n.endswith(".hip")})
        for d in ("old", "new"):
            os.makedirs(os.path.join(tmp, d))
        # both maps share the pool: at most this many hipcc run at once
        with concurrent.futures.ThreadPoolExecutor(max(1, min(8, (os.cpu_count() or 2) // 2))) as pool:
            olds = pool.map(lambda f: disassemble(os.path.join(base_dir, CSRC), f, os.path.join(tmp, "old")), files)
            news = pool.map(lambda f: disassemble(os.path.join(ROOT, CSRC), f, os.path.join(tmp, "new")), files)
            pairs = list(zip(files, olds, news))
        for f, old, new in pairs:
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
