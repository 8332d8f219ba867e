"""Are the kernels of two sets of device-only assembly files the same? (dev tool: the check that
moving kernels between translation units changed no device code)

    hipcc <library flags> --cuda-device-only -S <unit> -o <unit>.s      # one per unit, old and new
    python tools/isa_same.py old.s [old2.s ...] -- new.s [new2.s ...]

Every kernel (.amdhsa_kernel) must appear exactly once on each side, with the same registers,
scratch and LDS (the fields tools/isa_stats.py prints) and the same instruction stream once what
depends on a function's position in its file is normalised: comments, and the function index in
.LBB<n>_<m> labels and .Lfunc_* symbols.  Exit status 1 and a unified diff per kernel otherwise.
"""
import difflib
import re
import sys

FIELDS = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "private_segment_fixed_size",
          "group_segment_fixed_size")


def kernels(paths):
    """name -> (descriptor fields, normalised instruction lines); kernels seen twice in `dup`"""
    out, dup = {}, []
    for path in paths:
        s = open(path).read()
        for meta in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", s, re.S):
            name = meta.group(1)
            info = {}
            for k in FIELDS:
                mm = re.search(r"\.amdhsa_" + k + r"\s+(\d+)", meta.group(2))
                info[k] = int(mm.group(1)) if mm else None
            beg = re.search(r"^" + re.escape(name) + r":", s, re.M)
            end = s.find(".Lfunc_end", beg.end())
            body = []
            for line in s[beg.end():end].split("\n"):
                line = line.split(";")[0].rstrip()
                line = re.sub(r"\.LBB\d+_", ".LBB_", line)
                line = re.sub(r"\.L(func_\w+?|tmp)\d+", r".L\1", line)
                if line.strip():
                    body.append(line)
            if name in out:
                dup.append(name)
            out[name] = (info, body)
    return out, dup


def main(argv):
    if "--" not in argv:
        raise SystemExit(__doc__)
    cut = argv.index("--")
    old, dup_old = kernels(argv[:cut])
    new, dup_new = kernels(argv[cut + 1:])
    bad = 0
    for name in dup_old + dup_new:
        print("more than once:", name)
        bad += 1
    for name in sorted(set(old) ^ set(new)):
        print("only in the", "old" if name in old else "new", "files:", name)
        bad += 1
    for name in sorted(set(old) & set(new)):
        (io, bo), (inew, bn) = old[name], new[name]
        if io != inew:
            print("descriptor differs:", name, io, inew)
            bad += 1
        if bo != bn:
            print("instructions differ:", name)
            sys.stdout.writelines(l + "\n" for l in list(difflib.unified_diff(bo, bn, "old", "new", lineterm=""))[:80])
            bad += 1
    n_instr = sum(len(b) for _, b in new.values())
    print(f"{len(old)} kernels old, {len(new)} new, {n_instr} lines compared, {bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
