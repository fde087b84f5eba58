"""usage: isa_compare.py parent.s new.s [family prefix ...] -- the register / spill / scratch / occupancy / code-length listing of
kernel families from two `hipcc -S --cuda-device-only` dumps of the whole library, the way profiles/r10_selects_isa.txt and
r12_loops_isa.txt list them, and the instantiations that break the conditions (spilled VGPRs and scratch bytes not above, occupancy
not below the parent's).  The families are name prefixes such as `k_hess_pairs<` `k_jac_sweep<`; without any, the four spectrum
kernel families (k_spectrum, k_spectrum_fused, k_forward_pairs, k_spectrum_rows)."""
import re
import subprocess
import sys

FAMILIES = ("k_spectrum<", "k_spectrum_fused<", "k_forward_pairs<", "k_spectrum_rows<")


def kernels(path):
    text = open(path).read()
    out, order = {}, []
    for m in re.finditer(r"^(_ZN4tsff\w+):.*?^; Occupancy:\s*(\d+)", text, re.M | re.S):
        name, body = m.group(1), m.group(0)
        if name in out:
            continue
        g = lambda pat: int(re.search(pat, body).group(1))
        meta = text[re.search(r"^\s*\.name:\s+%s$" % re.escape(name), text, re.M).start():][:4000]
        gm = lambda pat: int(re.search(pat, meta).group(1))
        insts = "\n".join(l.split(";")[0].strip() for l in body.split("\n")[1:] if l.startswith("\t") and not l.strip().startswith((".", ";")))
        out[name] = dict(vgpr=g(r"; NumVgprs:\s*(\d+)"), sgpr=g(r"; TotalNumSgprs:\s*(\d+)"), occ=int(m.group(2)), code=g(r"; codeLenInByte = (\d+)"),
                         spillv=gm(r"\.vgpr_spill_count:\s*(\d+)"), spills=gm(r"\.sgpr_spill_count:\s*(\d+)"),
                         scratch=gm(r"\.private_segment_fixed_size:\s*(\d+)"), text=re.sub(r"\.LBB\d+_", ".LBB_", insts))
        order.append(name)
    return out, order


def main():
    a, oa = kernels(sys.argv[1])
    b, ob = kernels(sys.argv[2])
    def by_name(d, order):   # (keyed by the demangled name without its argument list: k_fused_prep gained an argument)
        dem = subprocess.run(["c++filt"], input="\n".join(order), capture_output=True, text=True, check=True).stdout.split("\n")
        names = [re.sub(r"^(void )?tsff::", "", x).split("(")[0] for x in dem[:len(order)]]
        return {n: d[m] for n, m in zip(names, order)}, names
    a, oa = by_name(a, oa)
    b, ob = by_name(b, ob)
    short = {m: m for m in oa}
    families = tuple(sys.argv[3:]) or FAMILIES
    these = "the four families" if families == FAMILIES else "the families " + " ".join(families)
    print("kernels: parent %d, new %d, same names (without argument lists) in the same order: %s" % (len(oa), len(ob), oa == ob))
    print("same set of names: %s" % (sorted(oa) == sorted(ob)))
    fam = [m for m in oa if short[m].startswith(families)]
    rest = [m for m in oa if m not in fam]
    print("kernels outside %s with different text:" % these, ", ".join(m for m in rest if a[m]["text"] != b[m]["text"]) or "none")
    print("kernels outside %s: %d, with different text: %d" % (these, len(rest), sum(a[m]["text"] != b[m]["text"] for m in rest)))
    print("kernels of %s: %d, with identical text: %d" % (these, len(fam), sum(a[m]["text"] == b[m]["text"] for m in fam)))
    print()
    print("%-52s %9s %9s %9s %7s %10s %5s %15s" % ("instantiation (parent -> new)", "VGPRs", "SGPRs", "spillV", "spillS", "scratch B", "occ", "codeLenInByte"))
    broken = []
    f = lambda x, y: str(x) if x == y else "%d->%d" % (x, y)
    for m in sorted(fam, key=lambda m: short[m]):
        p, n = a[m], b[m]
        same = "  (identical text)" if p["text"] == n["text"] else ""
        print("%-52s %9s %9s %9s %7s %10s %5s %15s%s" % (short[m], f(p["vgpr"], n["vgpr"]), f(p["sgpr"], n["sgpr"]), f(p["spillv"], n["spillv"]),
                                                       f(p["spills"], n["spills"]), f(p["scratch"], n["scratch"]), f(p["occ"], n["occ"]),
                                                       f(p["code"], n["code"]), same))
        if n["spillv"] > p["spillv"] or n["scratch"] > p["scratch"] or n["occ"] < p["occ"]:
            broken.append(short[m])
    print()
    print("conditions (spilled VGPRs and scratch bytes not above, occupancy not below the parent's) broken by:", ", ".join(broken) or "none")


if __name__ == "__main__":
    main()
