"""Static check of the hand-written vector-memory requests of the configs[3] sampler (project_rolling, k_form_factor_2d.inc).

The sampler requests the lines that enter its rolling window with `global_load` instructions written in inline assembly, one sample
ahead of their use, and waits for them with its own `s_waitcnt vmcnt(n)`.  The compiler does not know that a request's destination
registers hold nothing until the data has arrived: correctness rests on NO instruction touching them between the request and a wait
that covers it.  A first version violated that for odd table sizes (copies in front of a tail's wait) and failed intermittently; this
test reads the device assembly of every 2-D instantiation the library launches (1 to 4 ion species) and proves the property for every
hand-written request (a `global_load` between the compiler's ;;#ASMSTART / ;;#ASMEND markers) on every path:

    from the request, follow the control-flow graph -- fall-through, branch targets, loop back edges -- until an `s_waitcnt vmcnt(n)`
    with n <= the number of vector-memory loads issued after the request on that path; no instruction on the way may read or write
    one of the request's destination registers.  Control flow the walk cannot follow (indirect jumps, calls, unknown labels) fails.

The LDS-resident forms (<N, true, 4, *>) read the table from LDS and must carry no hand-written request (one added later is noticed
here and needs the walk).  Needs hipcc (cross-compiles without a GPU): one compile of all instantiations, about 20 s."""
import os
import re

import pytest

import isa

_FWD = "template __global__ void tsff::k_form_factor_2d<{n}, {lds}, {g}, {save}>(tsff::KStatic, const double*, const double*, int, double, double, int, long, long, double*, double*);"
_ADJ = "template __global__ void tsff::k_form_factor_2d_adj<{n}, {lds}, {g}>(tsff::KStatic, const double*, const double*, int, double, double, int, long, long, const double*, double*, double*, const double*);"
# name -> (explicit instantiation, mangled-name prefix); the forms tsff_api.inc launches: N = 1..4, tables through L1/L2 (false, 1)
# or resident in LDS (true, 4), with and without projection records
KERNELS = {}
for _n in (1, 2, 3, 4):
    for _lds, _g in (("false", 1), ("true", 4)):
        _b = "1" if _lds == "true" else "0"
        for _save in ("false", "true"):
            KERNELS[f"k_form_factor_2d<{_n}, {_lds}, {_g}, {_save}>"] = (
                _FWD.format(n=_n, lds=_lds, g=_g, save=_save), f"_ZN4tsff16k_form_factor_2dILi{_n}ELb{_b}ELi{_g}ELb{1 if _save == 'true' else 0}E")
        KERNELS[f"k_form_factor_2d_adj<{_n}, {_lds}, {_g}>"] = (_ADJ.format(n=_n, lds=_lds, g=_g), f"_ZN4tsff20k_form_factor_2d_adjILi{_n}ELb{_b}ELi{_g}E")


@pytest.fixture(scope="module")
def assembly():
    """device assembly of every instantiation of KERNELS, one compile"""
    return isa.compile_assembly(v[0] for v in KERNELS.values())


def _regs(tok):
    """'v[8:11]' -> {8, 9, 10, 11}; 'v47' -> {47}; anything else -> empty"""
    m = re.fullmatch(r"v\[(\d+):(\d+)\]", tok)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.fullmatch(r"v(\d+)", tok)
    return {int(m.group(1))} if m else set()


def _touched(args):
    out = set()
    for tok in re.findall(r"v\[\d+:\d+\]|v\d+", args):
        out |= _regs(tok)
    return out


_VMEM_LOAD = ("global_load", "buffer_load", "flat_load", "scratch_load")


def _parse(asm):
    """instructions (opcode, operands, inside inline assembly) and label -> index of one or more functions in order"""
    insts, labels, in_asm = [], {}, False
    for l in asm.split("\n"):
        if ";;#ASMSTART" in l:
            in_asm = True
        elif ";;#ASMEND" in l:
            in_asm = False
        t = l.split(";")[0].strip()
        if not t:
            continue
        m = re.match(r"^([.\w$]+):", t)
        if m:
            labels[m.group(1)] = len(insts)
            continue
        if t.startswith("."):
            continue
        p = t.split(None, 1)
        insts.append((p[0], p[1] if len(p) > 1 else "", in_asm))
    return insts, labels


def _successors(insts, labels, i):
    op, args, _ = insts[i]
    if op in ("s_endpgm", "s_endpgm_saved"):
        return []
    if op.startswith("s_setpc") or op.startswith("s_swappc") or op.startswith("s_call") or op.startswith("s_cbranch_g_fork") \
            or op.startswith("s_cbranch_join") or op.startswith("s_rfe"):
        raise AssertionError(("control flow the walk cannot follow", i, op, args))
    if op == "s_branch" or op.startswith("s_cbranch"):
        target = args.split(",")[0].strip()
        if target not in labels:
            raise AssertionError(("branch to an unknown label", i, op, args))
        succ = [labels[target]] if op == "s_branch" else [i + 1, labels[target]]
    else:
        succ = [i + 1]
    for j in succ:
        if j >= len(insts):
            raise AssertionError(("control flow runs off the end of the function", i, op, args))
    return succ


def _vmcnt(op, args):
    if op == "s_waitcnt":
        m = re.search(r"vmcnt\((\d+)\)", args)
        return int(m.group(1)) if m else None
    if op == "s_waitcnt_vmcnt":
        m = re.search(r"(0x[0-9a-fA-F]+|\d+)\s*$", args)
        return int(m.group(1), 0) if m else None
    return None


def _check(asm):
    """Walk the control-flow graph from every hand-written request (see the module docstring); returns how many were checked."""
    insts, labels = _parse(asm)
    checked = 0
    for k, (op, args, in_asm) in enumerate(insts):
        if not (in_asm and op.startswith(_VMEM_LOAD)):
            continue
        dst = _regs(args.split(",")[0].strip())
        assert dst, ("a request without a vector destination", op, args)
        # state of a path: vector-memory loads issued since the request.  A node reached again with as many or more later loads
        # is dominated (a wait covers it at least as well), so every node is expanded a bounded number of times.
        best = {}
        stack = [(j, 0) for j in _successors(insts, labels, k)]
        while stack:
            i, later = stack.pop()
            if i in best and best[i] <= later:
                continue
            best[i] = later
            op2, args2, _ = insts[i]
            n = _vmcnt(op2, args2)
            if n is not None and n <= later:
                continue   # covered on this path
            if op2.startswith(_VMEM_LOAD):
                assert not (_regs(args2.split(",")[0].strip()) & dst), \
                    ("request overwritten before its data was waited for", (k, op, args), "->", (i, op2, args2))
                assert not (_touched(args2.split(",", 1)[1] if "," in args2 else "") & dst), \
                    ("a request's destination is read before a wait covers it", (k, op, args), "->", (i, op2, args2))
                later += 1
            elif _touched(args2) & dst:
                raise AssertionError(("a request's destination is touched before a wait covers it", (k, op, args), "->", (i, op2, args2)))
            stack.extend((j, later) for j in _successors(insts, labels, i))
        checked += 1
    return checked


def _hand_written_requests(asm):
    insts, _ = _parse(asm)
    return sum(1 for op, _, in_asm in insts if in_asm and op.startswith(_VMEM_LOAD))


@pytest.mark.skipif(not os.path.exists(isa.HIPCC), reason="needs hipcc")
@pytest.mark.parametrize("name", sorted(KERNELS))
def test_request_registers_are_untouched_until_waited_for(assembly, name):
    fn = isa.function(assembly, KERNELS[name][1], end=".Lfunc_end")[1]
    n = _check(fn)
    if ", true, 4" in name:   # LDS-resident table: no hand-written requests (one added later needs this walk)
        assert n == 0 and _hand_written_requests(fn) == 0, n
    else:
        assert n >= 8 * 12, n   # eight walk forms (four in flight x two samples x six requests... at least twelve per loop)


_EXIT_HAZARD = """_ZN4tsff4testEv:
.LBB0_1:
\ts_waitcnt vmcnt(0)
\tv_add_f64 v[6:7], v[6:7], v[4:5]
\t;;#ASMSTART
\tglobal_load_dwordx2 v[4:5], v1, s[2:3]
\t;;#ASMEND
\ts_add_u32 s0, s0, -1
\ts_cmp_lg_u32 s0, 0
\ts_cbranch_scc1 .LBB0_1
%s\tv_mov_b64 v[8:9], v[4:5]
\ts_endpgm
.Lfunc_end0:
"""


def test_check_follows_requests_past_the_loop_exit():
    """The back edge reaches a covering wait, the exit path reads the request's destination without one: must be rejected (the
    innermost-loop walk this check replaces accepted it).  With a wait on the exit path the same code passes."""
    with pytest.raises(AssertionError, match="touched before a wait"):
        _check(_EXIT_HAZARD % "")
    assert _check(_EXIT_HAZARD % "\ts_waitcnt vmcnt(0)\n") == 1


def test_check_fails_on_control_flow_it_cannot_follow():
    bad = _EXIT_HAZARD.replace("s_cbranch_scc1 .LBB0_1", "s_setpc_b64 s[4:5]") % ""
    with pytest.raises(AssertionError, match="cannot follow"):
        _check(bad)
