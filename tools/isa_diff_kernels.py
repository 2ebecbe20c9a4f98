"""Dev tool: per-kernel diff of two gfx950 assembly listings of one translation unit -- which kernels of the parent are still
instruction for instruction (and kernel descriptor for kernel descriptor) what they were, which differ, which are new.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -x hip --cuda-device-only -S \
          [-Rpass-analysis=kernel-resource-usage] instantavatar_amd/csrc/ia_field.hip -o new.s       (the same on the parent: old.s)
    python tools/isa_diff_kernels.py old.s new.s [--rename REGEX REPLACEMENT]

Comments and the numbering of local labels (`.LBB12_3`: the function's index in the unit) are not code and are normalised away.
`--rename` maps the new listing's symbol names onto the parent's where a kernel only gained a template parameter, e.g.
    --rename '(k_encode_xcdILi\\d+)ELi3EE' '\\1EE'          k_encode_xcd<L, 3> of this tree against k_encode_xcd<L> of its parent
"""
import argparse
import re


def listing(path, rename):
    text = open(path).read()
    norm = lambda s: re.sub(r"\.L(BB|tmp|func_begin|JTI)\d+_", r".L\1N_", rename(s))
    code, cur = {}, None
    for ln in text.splitlines():
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            cur = norm(m.group(1))
            code[cur] = []
        elif cur is not None:
            if ln.startswith(".Lfunc_end"):
                cur = None
            else:
                ln = norm(ln.split(";")[0]).rstrip()
                if ln:
                    code[cur].append(ln)
    desc = {norm(m.group(1)): norm(m.group(2)) for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S)}
    return code, desc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rename", nargs=2, metavar=("REGEX", "REPLACEMENT"), default=None)
    a = ap.parse_args()
    ren = (lambda s: re.sub(a.rename[0], a.rename[1], s)) if a.rename else (lambda s: s)
    oc, od = listing(a.old, lambda s: s)
    nc, nd = listing(a.new, ren)
    same = [k for k in oc if k in nc and oc[k] == nc[k] and od.get(k) == nd.get(k)]
    print("%d functions in %s, %d in %s" % (len(oc), a.old, len(nc), a.new))
    print("identical (instructions and kernel descriptor): %d" % len(same))
    for title, names in (("different", [k for k in oc if k in nc and k not in same]), ("missing", [k for k in oc if k not in nc]),
                         ("new", [k for k in nc if k not in oc])):
        print("%s: %d" % (title, len(names)))
        for k in names:
            print("    %s   (%d instructions%s)" % (k, len(nc.get(k, oc.get(k))), "" if k not in oc or k not in nc else " against %d" % len(oc[k])))


if __name__ == "__main__":
    main()
