"""Did the device code change? Compare two sets of device assembly files, e.g. the search
sources before / after a refactor, built with the Makefile's FLAGS:

    hipcc $FLAGS --cuda-device-only -S search_mx.hip -o old/search_mx.s   (every search file)
    python tools/isa_diff.py old/ new/ [--resources]

Per kernel: the function body (its label to .Lfunc_end) and its .amdhsa_kernel block, with
comments stripped, .LBB<n>_ labels renumbered and the kernel's own mangled name replaced, are
hashed; the two multisets of hashes are compared. Kernel names play no part (a template
signature may change), and nothing is looked for in the code: it is the same or it is not.
Exit status 0 when the multisets are equal. --resources adds the .amdhsa register, scratch
and LDS lines of the kernels on either side only."""
import collections
import hashlib
import os
import re
import subprocess
import sys

RES = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "private_segment_fixed_size",
       "group_segment_fixed_size")


def files(arg):
    if os.path.isdir(arg):
        return sorted(os.path.join(arg, f) for f in os.listdir(arg) if f.endswith(".s"))
    return [arg]


def kernels(path):
    """{mangled name: (normalised text, {resource: value})} of one assembly file"""
    lines = open(path).read().split("\n")
    desc, label = {}, {}
    for i, l in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)
        if m:
            desc[m.group(1)] = i
        m = re.match(r"([A-Za-z_$][\w$.]*):", l)
        if m:
            label.setdefault(m.group(1), i)
    out = {}
    for name, k0 in desc.items():
        start = label[name]
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        k1 = next(i for i in range(k0, len(lines)) if ".end_amdhsa_kernel" in lines[i])
        body, labels, res = [], {}, {}
        for l in lines[start:end] + lines[k0:k1 + 1]:
            l = re.sub(r"\s*(;|//).*$", "", l).strip()
            if not l:
                continue
            l = l.replace(name, "KERNEL")
            l = re.sub(r"\.LBB\d+_(\d+)", lambda m: labels.setdefault(m.group(1), ".L%d" % len(labels)), l)
            m = re.match(r"\.amdhsa_(\w+)\s+(\S+)", l)
            if m and m.group(1) in RES:
                res[m.group(1)] = m.group(2)
            body.append(l)
        out[name] = ("\n".join(body), res)
    return out


def load(arg):
    ks = {}
    for f in files(arg):
        for name, v in kernels(f).items():
            ks[(os.path.basename(f), name)] = v
    return ks


def demangle(names):
    if not names:
        return []
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return r.stdout.strip().split("\n")


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    old, new = load(args[0]), load(args[1])
    h = lambda v: hashlib.sha256(v[0].encode()).hexdigest()
    ho = collections.Counter(h(v) for v in old.values())
    hn = collections.Counter(h(v) for v in new.values())
    print("%d kernels (%d distinct bodies) before, %d (%d) after" % (
        len(old), len(ho), len(new), len(hn)))
    only_old = ho - hn
    only_new = hn - ho
    for label, side, only in (("before only", old, only_old), ("after only", new, only_new)):
        keys = [k for k, v in sorted(side.items()) if h(v) in only]
        for k, d in zip(keys, demangle([k[1] for k in keys])):
            line = "%s: %s %s" % (label, k[0], re.sub(r"^void |\(.*$", "", d.replace("(anonymous namespace)::", "")))
            if "--resources" in sys.argv:
                line += " " + " ".join("%s=%s" % kv for kv in sorted(side[k][1].items()))
            print(line)
    same = not only_old and not only_new
    print("the device code is %s" % ("the same" if same else "NOT the same"))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
