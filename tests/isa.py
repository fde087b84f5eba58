"""Shared helpers of the static (no GPU) checks that read device assembly: cross-compile explicit kernel instantiations, cut one
function out, find its innermost loops, read the register and scratch figures of its metadata."""
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def compile_assembly(instantiations, root=ROOT, defines=()):
    """device assembly of the explicit instantiations (lines of C++) from the sources under root, one compile"""
    with tempfile.TemporaryDirectory() as d:
        src, out = os.path.join(d, "all.hip"), os.path.join(d, "all.s")
        open(src, "w").write('#define TSFF_NO_API\n#include "%s"\n%s\n' % (os.path.join(root, "tsadar_amd", "csrc", "tsff_kernels.hip"),
                                                                          "\n".join(instantiations)))
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-I" + os.path.join(root, "include"),
                        *defines, "-o", out, src], check=True, stderr=subprocess.DEVNULL)
        return open(out).read()


def function(asm, prefix, end="; Occupancy:"):
    """(mangled name, assembly) of the one function whose mangled name starts with prefix, up to the first line that starts with
    `end`: the end of its resource comments, or `.Lfunc_end` for the instructions alone"""
    lines = asm.split("\n")
    starts = [i for i, l in enumerate(lines) if l.startswith(prefix) and re.match(r"^_ZN4tsff\w+:", l)]
    assert len(starts) == 1, (prefix, len(starts))
    s = starts[0]
    e = next(i for i in range(s, len(lines)) if lines[i].startswith(end))
    return re.match(r"^(\w+):", lines[s]).group(1), "\n".join(lines[s:e + 1])


def innermost_loops(body):
    """(instructions, spans) of a function: its instruction lines, and (first, last) index of every innermost loop -- from a label
    to the last backward branch to it, with no other backward branch's target strictly inside"""
    insts, labels = [], {}
    for l in body.split("\n"):
        t = l.split(";")[0].strip()
        if not t:
            continue
        m = re.match(r"^([.\w$]+):", t)
        if m:
            labels[m.group(1)] = len(insts)
            continue
        if not t.startswith("."):
            insts.append(t)
    spans = {}
    for i, t in enumerate(insts):
        p = t.split(None, 1)
        if (p[0] == "s_branch" or p[0].startswith("s_cbranch")) and len(p) > 1:
            tgt = labels.get(p[1].split(",")[0].strip())
            if tgt is not None and tgt <= i:
                spans[tgt] = max(spans.get(tgt, i), i)
    inner = [(s, e) for s, e in spans.items() if not any((s2, e2) != (s, e) and s <= s2 and e2 <= e for s2, e2 in spans.items())]
    return insts, sorted(inner)


def resources(asm, prefixes):
    """name -> (spilled VGPRs, scratch bytes, occupancy) of every kernel of prefixes (name -> mangled-name prefix), from the kernel
    metadata (`.vgpr_spill_count`, `.private_segment_fixed_size`) and the `; Occupancy:` comment"""
    out = {}
    for name, prefix in prefixes.items():
        mangled, body = function(asm, prefix)
        meta = asm[re.search(r"^\s*\.name:\s+%s$" % re.escape(mangled), asm, re.M).start():]
        spill = int(re.search(r"\.vgpr_spill_count:\s*(\d+)", meta).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", meta).group(1))
        occ = int(re.search(r"; Occupancy:\s*(\d+)", body).group(1))
        out[name] = (spill, scratch, occ)
    return out
