"""Static check of the scheduled order of the one-sweep kernel's angle loops (r13_sweep_sched; no GPU needed, one compile).

The four angle loops of k_spectrum_fused<1, 0, false, true> -- the only instantiation that receives the order (kSweepSched, k_pairs.inc) --
are run through the committed issue model (scripts/issue_model.py) at the LDS latency calibrated on the device
(profiles/r13_ubench_lds_latency.txt).  Per loop:
* the modelled stall cycles of an iteration are at most half of the parent's figure for the same loop at the same latency (the parent's
  figures: the same script over the parent's assembly, recorded in profiles/r13_sweep_sched_model.txt);
* the VALU instructions are no more than the parent's 484 / 476 (general form, pair 0 / 1) and 354 / 358 (asymptotic form);
* no table read (ds_read_b128, ds_read2_b64, the exp table's ds_read_b64) is consumed sooner than ceil(latency / issue interval) VALU
  instructions after its request;
and the kernel keeps 0 spilled VGPRs, no scratch and two wavefronts per SIMD.

Mutation check (made when the order was written): with the scheduling barriers of pair_step_sched, fsqrt2_pair and fexp_finish_pair
compiled out, the compiler sinks the reads back to their uses and the first and third assertion fail."""
import os
import re
import sys

import pytest

import isa

sys.path.insert(0, os.path.join(isa.ROOT, "scripts"))
import issue_model  # noqa: E402

INSTANTIATION = "template __global__ void tsff::k_spectrum_fused<1, 0, false, true>(tsff::KStatic, tsff::KCall, int, int, const double*);"
PREFIX = issue_model.HEADLINE
PARENT_VALU = {("general", 0): 484, ("general", 1): 476, ("far", 0): 354, ("far", 1): 358}
RECORD = os.path.join(isa.ROOT, "profiles", "r13_sweep_sched_model.txt")
LOOPS = sorted(PARENT_VALU)


def parent_figures(latency):
    """(kind, pair) -> (VALU, stall cycles) of the parent's loops at the calibrated latency, from the record"""
    text = open(RECORD).read()
    m = re.search(r"^== parent[^\n]*LDS latency ([\d.]+)[^\n]*==\n(.*?)(?=^== )", text, re.M | re.S)
    assert m and float(m.group(1)) == latency, "the record's parent section is not at the calibrated latency"
    out = {}
    for g in re.finditer(r"\((\w+), pair (\d)\): \d+ instructions, VALU (\d+),.*?stall cycles ([\d.]+) =", m.group(2), re.S):
        out[g.group(1), int(g.group(2))] = (int(g.group(3)), float(g.group(4)))
    return out


@pytest.fixture(scope="module")
def assembly():
    return isa.compile_assembly([INSTANTIATION])


@pytest.fixture(scope="module")
def figures(assembly):
    return issue_model.angle_loop_figures(assembly, PREFIX, issue_model.lds_latency(), issue_model.constants())


def test_latency_is_the_calibrated_one():
    assert os.path.exists(issue_model.LDS_LATENCY_FILE)
    assert issue_model.lds_latency() != issue_model.ASSUMED_LDS_LATENCY or "model latency: 64" in open(issue_model.LDS_LATENCY_FILE).read()


def test_record_holds_the_parents_counts():
    parent = parent_figures(issue_model.lds_latency())
    assert {k: v[0] for k, v in parent.items()} == PARENT_VALU


@pytest.mark.parametrize("loop", LOOPS)
def test_stall_cycles_at_most_half_of_the_parents(figures, loop):
    parent = parent_figures(issue_model.lds_latency())[loop][1]
    f = figures[loop]
    print("%s pair %d: stall cycles %.1f (LDS %.1f, VALU %.1f), parent %.1f" % (loop + (f["stall"], f["stall_lds"], f["stall_valu"], parent)))
    assert f["stall"] <= 0.5 * parent, (loop, f["stall"], parent)


@pytest.mark.parametrize("loop", LOOPS)
def test_no_more_valu_instructions_than_the_parent(figures, loop):
    print("%s pair %d: VALU %d, parent %d" % (loop + (figures[loop]["valu"], PARENT_VALU[loop])))
    assert figures[loop]["valu"] <= PARENT_VALU[loop], (loop, figures[loop]["valu"])


@pytest.mark.parametrize("loop", LOOPS)
def test_table_reads_are_covered(figures, loop):
    need = issue_model.min_distance(issue_model.lds_latency(), issue_model.constants())
    table = [r for r in figures[loop]["reads"] if r["table"]]
    print("%s pair %d: VALU instructions between a table read and its first use %s, needed %d" % (loop + ([r["distance"] for r in table], need)))
    assert len(table) == (8 if loop[0] == "far" else 14), (loop, len(table))   # 2 x (Hermite cell 2, exp 1, W 1 | + Z' 2, exp 1)
    assert all(r["distance"] is not None and r["distance"] >= need for r in table), (loop, [(r["op"], r["distance"]) for r in table], need)


def test_no_spill_no_scratch_two_wavefronts(assembly):
    assert isa.resources(assembly, {"k": PREFIX})["k"] == (0, 0, 2)
