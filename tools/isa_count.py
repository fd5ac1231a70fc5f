"""Instruction mix of device kernels from hipcc's -save-temps assembly: total, VALU, fp64 VALU, MFMA, LDS, global, barriers.
usage: python tools/isa_count.py <file.s> <kernel-name-substring> [...]   (static counts; loops are counted once)
       python tools/isa_count.py diff <A.s> <B.s>                         (which kernels' mnemonic sequences differ)"""
import sys
from collections import Counter


def kernels(path):
    cur, out = None, {}
    for line in open(path):
        if line.startswith("_Z") and ":" in line:
            cur = line.split(":")[0]
            out[cur] = []
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur and line.startswith("\t"):
            t = line.strip()
            if t and not t.startswith((".", ";")):
                out[cur].append(t.split()[0])
    return out


def diff(path_a, path_b):
    """per kernel of two assembly files: identical mnemonic sequence, or the instruction counts of both sides"""
    a, b = kernels(path_a), kernels(path_b)
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print("%-9s %s" % ("only in A" if name in a else "only in B", name))
        elif a[name] == b[name]:
            print("%-9s %s" % ("identical", name))
        else:
            print("%-9s %s  (%d -> %d instructions)" % ("DIFFERENT", name, len(a[name]), len(b[name])))


if __name__ == "__main__":
    if sys.argv[1] == "diff":          # python tools/isa_count.py diff A.s B.s
        diff(sys.argv[2], sys.argv[3])
        sys.exit(0)
    ks = kernels(sys.argv[1])
    for name, ins in ks.items():
        if not any(p in name for p in sys.argv[2:]):
            continue
        c = Counter(ins)
        def n(pred):
            return sum(v for k, v in c.items() if pred(k))
        print("%s\n  total %d  VALU %d (fp64 %d)  MFMA %d  LDS %d  global %d  s_barrier %d  s_waitcnt %d" % (
            name, len(ins), n(lambda k: k.startswith("v_") and not k.startswith("v_mfma")),
            n(lambda k: k.startswith("v_") and "f64" in k and not k.startswith("v_mfma")),
            n(lambda k: k.startswith("v_mfma")), n(lambda k: k.startswith("ds_")), n(lambda k: k.startswith("global_")),
            c.get("s_barrier", 0), c.get("s_waitcnt", 0)))
        print("  most frequent:", ", ".join("%s x%d" % kv for kv in c.most_common(12)))
