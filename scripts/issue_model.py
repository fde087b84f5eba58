"""usage: issue_model.py [--lds-latency C] [--kernel PREFIX] [--all-loops] kernels.s -- a static, in-order issue model of ONE wavefront
over the innermost loops of a kernel, from its device assembly (`hipcc -S --cuda-device-only`, or tests/isa.py's compile_assembly).

Per loop it prints
* for every LDS read, the VALU instructions between the read and the first instruction that uses its result, in program order;
* the modelled cycles of one iteration without stalls and with them;
* the stall cycles by cause: waiting for an LDS (or scalar-memory) result, waiting for the result of a VALU instruction.

The model.  Instructions issue in program order (the span of the loop as it is laid out: forward branches inside it are not taken).
A VALU instruction issues when the previous one's issue interval has passed and its register operands are ready; its result is ready
one dependent latency after its issue.  The intervals and latencies are not typed in here: they are read from the micro-benchmark
listing profiles/r03b_ubench_dep.txt (scripts/ubench_dep.hip) -- `v_fma_f64` with 8 independent chains of one wavefront for the issue
interval, with 1 chain for the dependent latency, `v_rcp_f64` the same way for v_rcp_f64 / v_rsq_f64.  An LDS read or scalar load is
requested when its address is ready and returns --lds-latency cycles later (profiles/r13_ubench_lds_latency.txt measures it; the
default below is an assumption until that file exists); the wavefront waits where the compiler's s_waitcnt lgkmcnt(n) tells it to,
until all but the last n requests have returned (LDS returns in order).  Scalar ALU, branch and wait instructions take no VALU issue
time.  One iteration is modelled from a state in which everything is ready: stalls carried around the back edge are not counted.
The model ranks schedules of the same instructions; the device's own figures are in profiles/."""
import argparse
import math
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import isa  # noqa: E402  (the helpers of the static checks: one definition of "function" and "innermost loop")

UBENCH_DEP = os.path.join(ROOT, "profiles", "r03b_ubench_dep.txt")
LDS_LATENCY_FILE = os.path.join(ROOT, "profiles", "r13_ubench_lds_latency.txt")
ASSUMED_LDS_LATENCY = 64.0
HEADLINE = "_ZN4tsff16k_spectrum_fusedILi1ELi0ELb0ELb1EE"


def constants(path=UBENCH_DEP):
    """issue interval and dependent latency (cycles of one wavefront) of the FP64 pipe and of v_rcp_f64, from the listing"""
    got = {}
    for l in open(path):
        m = re.match(r"(\w+)\s+chains\s+(\d+), (\d+) wavefront\(s\) per SIMD: ([\d.]+) cycles", l)
        if m:
            got[m.group(1), int(m.group(2)), int(m.group(3))] = float(m.group(4))
    fp64 = ("v_fma_f64", "v_mul_f64", "v_add_f64")
    return dict(issue=min(v for (op, ch, wf), v in got.items() if op in fp64 and wf == 1),
                dep=got["v_fma_f64", 1, 1], trans_issue=got["v_rcp_f64", 8, 1], trans_dep=got["v_rcp_f64", 1, 1])


def lds_latency(path=LDS_LATENCY_FILE):
    """the calibrated issue-to-use latency of a table read (the listing's `model latency:` line), or the assumption without the file"""
    if os.path.exists(path):
        m = re.search(r"^model latency:\s*([\d.]+)", open(path).read(), re.M)
        if m:
            return float(m.group(1))
    return ASSUMED_LDS_LATENCY


_REG = re.compile(r"\b([vsa])\[(\d+):(\d+)\]|\b([vsa])(\d+)\b|\b(vcc|exec|scc)\b")


def regs(operand):
    out = []
    for m in _REG.finditer(operand):
        if m.group(1):
            out += [(m.group(1), i) for i in range(int(m.group(2)), int(m.group(3)) + 1)]
        elif m.group(4):
            out.append((m.group(4), int(m.group(5))))
        else:
            out.append((m.group(6), 0))
    return out


def decode(t):
    """(mnemonic, registers written, registers read) of one instruction line"""
    p = t.split(None, 1)
    op, ops = p[0], [o.strip() for o in (p[1].split(",") if len(p) > 1 else [])]
    ops = [o for o in ops if not re.match(r"^(offset|offset0|offset1|row_mask|bank_mask|wave_sh|row_|quad_perm|bound_ctrl)", o.split(":")[0].split()[0])] if ops else ops
    rd = lambda xs: [r for o in xs for r in regs(o)]
    if op.startswith("v_cmp") and op.endswith("_e32"):
        return op, [("vcc", 0)], rd(ops)
    if op.startswith("ds_read") or op.startswith("s_load"):
        return op, regs(ops[0]), rd(ops[1:])
    if op.startswith(("ds_write", "global_store", "s_waitcnt", "s_cbranch", "s_branch", "s_cmp", "s_nop", "s_barrier")):
        return op, [], rd(ops) + ([("vcc", 0)] if "vcc" in op else [])
    if not ops:
        return op, [], []
    wr, src = regs(ops[0]), rd(ops[1:])
    if op.startswith(("v_fmac", "v_mac")) or "dpp" in op or "dpp" in t or "wave_shl" in t:
        src = src + wr     # (the destination is an operand too: accumulator, or DPP's `old`)
    if op.startswith("v_cndmask") and op.endswith("_e32"):
        src = src + [("vcc", 0)]
    return op, wr, src


def is_valu(op):
    return op.startswith("v_")


def is_trans(op):
    return op.startswith(("v_rcp_f64", "v_rsq_f64", "v_sqrt_f64"))


def is_table_read(k, dec):
    """the lookups' reads: the Hermite cell (ds_read_b128), the W / Z' pairs (ds_read2_b64) and the 2^(j/64) entry of the exp table --
    a ds_read_b64 whose address is (n & 63) << 3 plus a base, formed in the loop"""
    op, _, src = dec[k]
    if op in ("ds_read_b128", "ds_read2_b64"):
        return True
    if op != "ds_read_b64":
        return False
    def producer(r, before):
        for j in range(before - 1, -1, -1):
            if r in dec[j][1]:
                return j
        return None
    a = producer(src[0], k) if src else None
    if a is None or not dec[a][0].startswith("v_lshl_add_u32"):
        return False
    b = producer(dec[a][2][0], a)
    return b is not None and dec[b][0].startswith("v_and_b32")


def analyse(ops):
    """LDS reads of one loop body (list of instruction lines) with their distance to the first use, and its VALU count"""
    dec = [decode(t) for t in ops]
    n = len(dec)
    # --- distance, in VALU instructions, from every LDS read to the first use of its result
    reads = []
    for k, (op, wr, _) in enumerate(dec):
        if not op.startswith("ds_read"):
            continue
        w, dist, used = set(wr), 0, False
        for j in range(k + 1, n):
            if w & set(dec[j][2]):
                used = True
                break
            w -= set(dec[j][1])      # (overwritten before any use: the value is dead from here)
            if not w:
                break
            dist += is_valu(dec[j][0])
        reads.append(dict(op=op, index=k, distance=dist if used else None, table=is_table_read(k, dec)))
    return dict(reads=reads, valu=sum(is_valu(d[0]) for d in dec))


def model(ops, c, lat):
    """the in-order walk of one iteration, waiting at every s_waitcnt lgkmcnt(n) of the compiler"""
    dec = [decode(t) for t in ops]
    t, nostall, ready, kind_of = 0.0, 0.0, {}, {}
    inflight, stall = [], dict(lds=0.0, valu=0.0)
    for line, (op, wr, src) in zip(ops, dec):
        if op == "s_waitcnt":
            m = re.search(r"lgkmcnt\((\d+)\)", line)
            if m:
                keep = int(m.group(1))
                done = inflight[:len(inflight) - keep] if keep else inflight
                if done and max(done) > t:
                    stall["lds"] += max(done) - t
                    t = max(done)
                inflight = inflight[len(inflight) - keep:] if keep else []
            continue
        if is_valu(op) or op.startswith(("ds_read", "s_load", "ds_write")):
            need, kind = t, None
            for r in src:
                if ready.get(r, 0.0) > need:
                    need, kind = ready[r], kind_of.get(r, "valu")
            if need > t:
                stall[kind] += need - t
                t = need
        if is_valu(op):
            iv, dl = (c["trans_issue"], c["trans_dep"]) if is_trans(op) else (c["issue"], c["dep"])
            for r in wr:
                ready[r], kind_of[r] = t + dl, "valu"
            t += iv
            nostall += iv
        elif op.startswith(("ds_read", "s_load")):
            back = max([t + lat] + inflight[-1:])
            inflight.append(back)
            for r in wr:
                ready[r], kind_of[r] = back, "lds"
    return dict(cycles=t, nostall=nostall, stall_lds=stall["lds"], stall_valu=stall["valu"], stall=stall["lds"] + stall["valu"])


def loop_figures(ops, c, lat):
    a = analyse(ops)
    out = model(ops, c, lat)
    out.update(valu=a["valu"], reads=a["reads"], lds_reads=len(a["reads"]))
    return out


def angle_loops(body):
    """the angle loops of a pair-sweep kernel: the innermost loops with the lane exchange's `wave_shl:1` moves (tests/test_isa_loops.py)"""
    insts, inner = isa.innermost_loops(body)
    return [ops for ops in (insts[s:e + 1] for s, e in inner) if any("wave_shl:1" in t for t in ops)]


def loop_labels(loops):
    """(kind, pair) of the four angle loops of a kernel: the two with the fewest LDS reads are the asymptotic (`far`) form, and within
    a form the text has pair 0's loop in front of pair 1's"""
    n = [sum(t.startswith("ds_read") for t in ops) for ops in loops]
    far = sorted(range(len(loops)), key=lambda k: (n[k], k))[:len(loops) // 2]
    seen, out = {"far": 0, "general": 0}, []
    for k in range(len(loops)):
        kind = "far" if k in far else "general"
        out.append((kind, seen[kind]))
        seen[kind] += 1
    return out


def angle_loop_figures(asm, prefix, lat, c):
    """(kind, pair) -> figures of the four angle loops of the kernel whose mangled name starts with prefix"""
    loops = angle_loops(isa.function(asm, prefix)[1])
    return {lab: loop_figures(ops, c, lat) for lab, ops in zip(loop_labels(loops), loops)}


def report(asm, prefix, lat, c, all_loops=False, out=sys.stdout):
    name, body = isa.function(asm, prefix)
    if all_loops:
        insts, inner = isa.innermost_loops(body)
        loops = [insts[s:e + 1] for s, e in inner]
    else:
        loops = angle_loops(body)
    print("%s: %d loop(s); issue %.2f, dependent %.2f, v_rcp/rsq_f64 %.2f / %.2f, LDS issue-to-use %.1f cycles" %
          (name, len(loops), c["issue"], c["dep"], c["trans_issue"], c["trans_dep"], lat), file=out)
    figs = []
    for k, ops in enumerate(loops):
        f = loop_figures(ops, c, lat)
        figs.append(f)
        lab = "" if all_loops else " (%s, pair %d)" % loop_labels(loops)[k]
        print("loop %d%s: %d instructions, VALU %d, LDS reads %d" % (k, lab, len(ops), f["valu"], f["lds_reads"]), file=out)
        print("  VALU instructions before first use, per LDS read (* = table read): " +
              ", ".join(("%s%s" % ("-" if r["distance"] is None else r["distance"], "*" if r["table"] else "")) for r in f["reads"]), file=out)
        print("  cycles per iteration: %.0f without stalls, %.0f modelled (+%.1f %%); stall cycles %.1f = %.1f waiting for LDS + %.1f waiting for a VALU result" %
              (f["nostall"], f["cycles"], 100.0 * f["stall"] / f["nostall"], f["stall"], f["stall_lds"], f["stall_valu"]), file=out)
    return figs


def min_distance(lat, c):
    """VALU instructions that cover one LDS round trip at the issue rate of one wavefront"""
    return int(math.ceil(lat / c["issue"]))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("assembly")
    ap.add_argument("--lds-latency", type=float, default=None, help="issue-to-use cycles of an LDS read (default: the calibrated value of "
                    "profiles/r13_ubench_lds_latency.txt, %g without that file)" % ASSUMED_LDS_LATENCY)
    ap.add_argument("--kernel", default=HEADLINE, help="mangled-name prefix of the kernel (default: the headline instantiation)")
    ap.add_argument("--all-loops", action="store_true", help="every innermost loop, not only the angle loops")
    a = ap.parse_args()
    c = constants()
    lat = lds_latency() if a.lds_latency is None else a.lds_latency
    report(open(a.assembly).read(), a.kernel, lat, c, a.all_loops)
    print("a table read is covered by %d VALU instructions at this latency" % min_distance(lat, c))


if __name__ == "__main__":
    main()
