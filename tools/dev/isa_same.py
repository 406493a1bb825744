"""dev: do two builds hold the same device code?  Each side is one or more device assembly files (the Makefile's flags plus
--cuda-device-only -S, one file per .hip), sides separated by "--":
   python tools/dev/isa_same.py old/siftmi.s -- new/siftmi.s new/match.s new/host_pool.s
Per kernel symbol the instruction text (comments dropped, the function index in .LBB<i>_<j> and its like normalised) and
the .amdhsa_* descriptor block must be identical; exit status 1 and the differing names otherwise."""
import re, sys

def kernels(paths):
    body, desc = {}, {}
    for path in paths:
        fn = kd = None          # open function (symbol label .. .Lfunc_end) / open descriptor block, each (name, lines)
        for raw in open(path):
            t = raw.split(";")[0].strip()
            if not t: continue
            if t.startswith(".amdhsa_kernel "): kd = (t.split()[1], []); continue
            if kd:
                if t == ".end_amdhsa_kernel": desc.setdefault(kd[0], []).append("\n".join(kd[1])); kd = None
                else: kd[1].append(t)
                continue
            m = re.match(r"(_Z\w+):$", t)
            if m and not fn: fn = (m.group(1), []); continue
            if not fn: continue
            if t.startswith(".Lfunc_end"): body.setdefault(fn[0], []).append("\n".join(fn[1])); fn = None; continue
            fn[1].append(re.sub(r"\.L([A-Za-z_]+)\d+_(\d+)", r".L\1_\2", t))
    return {k: (body.get(k), v) for k, v in desc.items()}      # kernels: the symbols with a descriptor

args = sys.argv[1:]
cut = args.index("--")
old, new = kernels(args[:cut]), kernels(args[cut + 1:])
twice = [k for side in (old, new) for k, (b, d) in side.items() if b is None or len(b) != 1 or len(d) != 1]
gone, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
differ = sorted(k for k in set(old) & set(new) if old[k] != new[k])
for title, names in (("not compiled exactly once", twice), ("only in the first", gone), ("only in the second", added), ("differ", differ)):
    for k in names: print("%s: %s" % (title, k))
ok = not (twice or gone or added or differ)
print("isa_same: %d / %d kernels, %d instruction lines; %s" % (len(old), len(new), sum(b[0].count("\n") + 1 for b, d in new.values() if b),
                                                               "identical code and descriptors" if ok else "DIFFERENT"))
sys.exit(0 if ok else 1)
