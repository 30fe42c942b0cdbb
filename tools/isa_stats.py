"""Per-kernel instruction counts of a HIP source's gfx950 ISA (scratch / global / LDS traffic sites).

    python tools/isa_stats.py cadence_amd/csrc/ingest_kernel.hip [substring ...]

Compiles device-only to assembly (hipcc -S, with the library's flags: __graft_entry__.build) and counts,
per function, the scratch loads / stores (spills and private arrays), global loads / stores, LDS ops, scalar
loads (s_load_*: kernel arguments and constants) and register copies (v_mov_*): a quick check that a hot
kernel has no scratch traffic, and what its loops reload or copy, before spending GPU time on it.
"""
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def isa(src):
    out = os.path.join(tempfile.mkdtemp(), "k.s")
    # the machine scheduler of the shipped library: without it the counts are those of another schedule
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17",
                    "-mllvm", "-amdgpu-sched-strategy=max-ilp",
                    "-I" + os.path.join(HERE, "include"), "-I" + os.path.join(HERE, "cadence_amd", "csrc"),
                    "--cuda-device-only", "-S", "-o", out, src], check=True)
    return open(out).read()


def main():
    src, subs = sys.argv[1], sys.argv[2:]
    s = isa(src)
    pats = {"scratch_ld": r"\bscratch_load|buffer_load\w* v\d+, off, s\[0:3\]",
            "scratch_st": r"\bscratch_store|buffer_store\w* v\d+, off, s\[0:3\]",
            "global_ld": r"\bglobal_load", "global_st": r"\bglobal_store", "lds": r"\bds_", "calls": r"\bs_swappc|\bs_setpc",
            "s_load": r"\bs_load_dword|\bs_buffer_load_dword", "v_mov": r"\bv_mov_b(?:32|64)"}
    for m in re.finditer(r"^([_A-Za-z]\w*):[^\n]*\n(.*?)\.Lfunc_end", s, re.S | re.M):
        name, body = m.group(1), m.group(2)
        if subs and not any(k in name for k in subs):
            continue
        counts = " ".join(f"{k}={len(re.findall(p, body)):4d}" for k, p in pats.items())
        print(f"{name[:70]:70s} lines={body.count(chr(10)):6d} {counts}")


if __name__ == "__main__":
    main()
