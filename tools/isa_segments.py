"""Static instruction counts of kernels in a device assembly file, per segment between barriers.

    hipcc <the build's flags> --offload-device-only -S lbt_amd/csrc/conv_fused_bwd.hip -o bwd.s
    python tools/isa_segments.py bwd.s [name-filter ...]

One block per kernel whose demangled name contains every filter: a row per segment (the instructions
between two s_barrier, in program order; loops are fully unrolled in the fused conv kernels, so the static
count is what a wave issues on its longest path) with the VALU, SALU (s_nop and s_waitcnt apart), s_nop,
MFMA and memory (global / buffer / flat / scratch / LDS) instruction counts, then the totals and the
counts of the instructions the overflow counters are judged by: lane <-> scalar moves (v_readlane,
v_writelane, v_readfirstlane), self-maxima (v_max_f32 x, x, x: a canonicalisation) and scratch accesses.
"""
import re
import subprocess
import sys


def kernels(asm):
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    out, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^([A-Za-z_$.][\w$.]*):", line)
        if m:
            if m.group(1) in names:
                cur = out.setdefault(m.group(1), [])
            elif m.group(1).startswith(".Lfunc_end"):
                cur = None
            continue
        if cur is None:
            continue
        text = line.split(";")[0].strip()
        if text and not text.startswith("."):
            cur.append(text)
    return out


def kind(ins):
    op = ins.split()[0]
    if op == "s_nop":
        return "nop"
    if op.startswith("s_waitcnt") or op == "s_barrier":
        return "wait"
    if op.startswith(("s_load", "s_buffer_load", "global_", "buffer_", "flat_", "scratch_", "ds_")):
        return "mem"
    if op.startswith("v_mfma") or op.startswith("v_smfma"):
        return "mfma"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_"):
        return "salu"
    return "other"


def self_max(ins):
    m = re.match(r"v_max_f32(?:_e32|_e64)?\s+(\w+), (\w+), (\w+)$", ins)
    return bool(m) and m.group(2) == m.group(3)


def main():
    asm = open(sys.argv[1]).read()
    filt = sys.argv[2:]
    ks = kernels(asm)
    full = subprocess.run(["c++filt"], input="\n".join(ks), capture_output=True, text=True).stdout.splitlines()
    for name, dem in zip(ks, full):
        dem = re.sub(r"\(anonymous namespace\)::|lbt::", "", dem).split("(")[0]
        if not all(f in dem for f in filt):
            continue
        segs = [[]]
        for ins in ks[name]:
            if ins.startswith("s_barrier"):
                segs.append([])
            else:
                segs[-1].append(ins)
        print(dem)
        print("  %-8s %6s %6s %6s %6s %6s" % ("segment", "VALU", "SALU", "s_nop", "MFMA", "memory"))
        tot = dict(valu=0, salu=0, nop=0, mfma=0, mem=0)
        for i, seg in enumerate(segs):
            c = dict(valu=0, salu=0, nop=0, mfma=0, mem=0, wait=0, other=0)
            for ins in seg:
                c[kind(ins)] += 1
            for k in tot:
                tot[k] += c[k]
            print("  %-8d %6d %6d %6d %6d %6d" % (i, c["valu"], c["salu"], c["nop"], c["mfma"], c["mem"]))
        print("  %-8s %6d %6d %6d %6d %6d" % ("total", tot["valu"], tot["salu"], tot["nop"], tot["mfma"], tot["mem"]))
        body = ks[name]
        lane = sum(1 for i in body if i.startswith(("v_readlane", "v_writelane", "v_readfirstlane")))
        print("  lane<->scalar moves %d, self-maxima %d, scratch accesses %d, v_cmp %d, s_bcnt1 %d" % (
            lane, sum(self_max(i) for i in body), sum(1 for i in body if i.startswith("scratch_")),
            sum(1 for i in body if i.startswith("v_cmp")), sum(1 for i in body if i.startswith("s_bcnt1"))))


if __name__ == "__main__":
    main()
