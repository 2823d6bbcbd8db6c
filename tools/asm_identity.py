"""Per-kernel comparison of the device assembly of two source trees.

    python tools/asm_identity.py PARENT_TREE RESULT_TREE PARENT_FILES RESULT_FILES [-j N]

PARENT_FILES / RESULT_FILES: comma-separated .hip paths relative to each tree (a file split in several
is one name on the left and several on the right). Every file is compiled with the build's flags plus
``--offload-device-only -S``; a kernel's text is what stands between its label and its end label, with
labels, comments, directives (``.loc`` among them) and blank lines dropped and the function index taken
out of local branch targets (``.LBB12_3`` -> ``.LBB_3``: it numbers the functions of a file). Kernels are
matched by demangled name with the namespaces stripped. One line per kernel on stdout:

    IDENTICAL|DIFFERENT|ONLY_PARENT|ONLY_RESULT  instructions before  after  name

Exit status 0 only if the two kernel sets are equal and every kernel is identical.
"""
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lbt_amd import _build  # noqa: E402


def device_asm(tree, rel, tmp):
    out = os.path.join(tmp, "%s.s" % abs(hash((tree, rel))))
    flags = [f for f in _build.FLAGS if not f.startswith("-I")] + ["-I" + os.path.join(tree, "include")]
    cmd = [_build.HIPCC] + flags + ["--offload-device-only", "-S", os.path.join(tree, rel), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed on %s:\n%s" % (rel, r.stderr))
    with open(out) as f:
        return f.read()


def kernels(asm):
    """{mangled name: [instruction lines]} of one assembly file."""
    lines = asm.splitlines()
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    out, cur = {}, None
    for line in lines:
        m = re.match(r"^([A-Za-z_$.][\w$.]*):", line)
        if m:
            label = m.group(1)
            if label in names:
                cur = out.setdefault(label, [])
            elif label.startswith(".Lfunc_end"):
                cur = None
            continue
        if cur is None:
            continue
        text = line.split(";")[0].strip()
        if not text or text.startswith("."):
            continue
        cur.append(re.sub(r"\.LBB\d+_", ".LBB_", text))
    return out


def demangled(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return [re.sub(r"\(anonymous namespace\)::|lbt::", "", n) for n in out]


def tree_kernels(tree, files, tmp, jobs):
    with concurrent.futures.ThreadPoolExecutor(max_workers=jobs) as ex:
        asms = list(ex.map(lambda rel: device_asm(tree, rel, tmp), files))
    merged = {}
    for asm in asms:
        ks = kernels(asm)
        for name, full in zip(ks, demangled(list(ks))):
            if full in merged:
                raise RuntimeError("kernel twice in one tree: " + full)
            merged[full] = ks[name]
    return merged


def main():
    args = sys.argv[1:]
    jobs = 4
    if "-j" in args:
        i = args.index("-j")
        jobs = int(args[i + 1])
        del args[i:i + 2]
    ptree, rtree, pfiles, rfiles = args
    with tempfile.TemporaryDirectory() as tmp:
        before = tree_kernels(ptree, pfiles.split(","), tmp, jobs)
        after = tree_kernels(rtree, rfiles.split(","), tmp, jobs)
    bad = 0
    for name in sorted(set(before) | set(after)):
        b, a = before.get(name), after.get(name)
        verdict = "ONLY_RESULT" if b is None else "ONLY_PARENT" if a is None else "IDENTICAL" if a == b else "DIFFERENT"
        bad += verdict != "IDENTICAL"
        short = name.split("(")[0]
        print("%-11s %6s %6s %s" % (verdict, "-" if b is None else len(b), "-" if a is None else len(a), short))
    print("%d kernels before, %d after, %d not identical" % (len(before), len(after), bad), file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
