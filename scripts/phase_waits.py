"""Memory loads and the waits on them per phase of the step kernel, joined with the phase stamps.

    hipcc <product flags> -DZB_STAMPS -DZB_XG_MASK=0x01 --cuda-device-only -S -o stamps.s zb_engine.hip
    python scripts/phase_waits.py stamps.s <kernel symbol> [--stamps tests/diag_stamps.py's JSON ...] [--json OUT]

Beside isa_phases.py (instruction mix between the phase stamps) and isa_waits.py (loads and waits per
loop). Between consecutive stamps of a -DZB_STAMPS build, in text order:

  - the loads by class: scalar memory (s_load / s_buffer_load), global (global / flat / buffer),
    scratch, LDS (ds_*, bpermute included);
  - every s_waitcnt by the class of the youngest load its counter covers (vmcnt: global and scratch;
    lgkmcnt: scalar memory and LDS), with the distance in instructions from that load. A small
    distance is a round trip the wave sits out in full.

With --stamps (one or more outputs of tests/diag_stamps.py, e.g. 512 envs on one stream, where a wave
is alone on its SIMD, and 8192): per phase the cycles per call, and cycles - 4 x instructions. One
wave issues at most one instruction every 4 cycles, so for a straight-line phase, whose static
count is its executed count, that difference is what the wave spent not issuing: its waits. The
segments the compiler's block placement mixes or that hold loops (constraints, the solver) are
listed without the difference.

--audit (any build, stamps or not): the lane record's loads are volatile asm statements whose waits
are written by hand (zb_engine.hip lr_crb_issue / lr_crb_wait), and the compiler counts an asm load's
destination as written when the statement ends. Between each such statement and the next asm wait
on vmcnt, in text order, no compiler instruction may name a destination register: a copy, a spill
or a reuse there would read or lose data that has not landed. Exit status 1 if one does.

A segment is named after the stamp that ends it. Stamps drain lgkmcnt only (zb_stamp), so a vector
load in flight across a stamp stays in flight, as in the product build.
"""
import argparse
import json
import re

from isa_phases import NSTAMP, PHASES, stamp_slot
from isa_waits import CLASSES, classify

# phases that are straight-line code run once per substep: static count == executed count
STRAIGHT = ("feetech", "kinematics", "com_crb_M", "factor_M", "rne_bias", "solve_smooth", "forward_entry", "integrate")
# tests/diag_stamps.py spells one phase differently
STAMP_KEYS = {"step_end": "step_end(obs/reward/reset)"}


def instructions(text, name):
    i = text.find(name + ":")
    assert i >= 0, f"no symbol {name}"
    j = text.find(".Lfunc_end", i)
    ins = []
    for raw in text[i:j].split("\n")[1:]:
        l = raw.split(";")[0].strip()
        if not l or l.endswith(":") or l.startswith("."):
            continue
        ins.append(l)
    return ins


def segment_rows(ins):
    stamps = [k for k, l in enumerate(ins) if l.startswith("s_memtime")]
    slots = [stamp_slot(ins, k) for k in stamps]
    last = dict.fromkeys(CLASSES, None)  # index of the youngest load of each class, kernel-wide
    rows, prev = [], 0
    for k, slot in zip(stamps, slots):
        row = {"ends_at": PHASES[slot] if slot is not None else "?", "instructions": k - prev,
               "valu": sum(1 for x in ins[prev:k] if x.startswith("v_")),
               "loads": dict.fromkeys(CLASSES, 0), "waits": {c: [] for c in CLASSES}}
        for at in range(prev, k):
            op = ins[at].split()[0]
            c = classify(op)
            if c:
                row["loads"][c] += 1
                last[c] = at
            if op != "s_waitcnt":
                continue
            for cnt, classes in (("vmcnt", ("global", "scratch")), ("lgkmcnt", ("smem", "lds"))):
                if not re.search(cnt + r"\(\d+\)", ins[at]):
                    continue
                young = [(last[x], x) for x in classes if last[x] is not None]
                if young:
                    y, what = max(young)
                    row["waits"][what].append(at - y - 1)
        rows.append(row)
        prev = k
    return rows


def audit(text, name):
    """[(load statement's line, offending instruction)], and the number of asm load statements."""
    i = text.find(name + ":")
    assert i >= 0, f"no symbol {name}"
    lines = text[i:text.find(".Lfunc_end", i)].split("\n")
    in_asm, regs, found, nloads, at = False, set(), [], 0, None

    def named(code):
        out = {int(r) for r in re.findall(r"\bv(\d+)\b", code)}
        for lo, hi in re.findall(r"\bv\[(\d+):(\d+)\]", code):
            out |= set(range(int(lo), int(hi) + 1))
        return out

    for k, raw in enumerate(lines):
        if "#ASMSTART" in raw:
            in_asm = True
            continue
        if "#ASMEND" in raw:
            in_asm = False
            continue
        code = raw.split(";")[0].strip()
        if not code or code.endswith(":") or code.startswith("."):
            continue
        if in_asm:
            m = re.match(r"(?:global|buffer|flat)_load_dword\S*\s+(v\d+|v\[\d+:\d+\])", code)
            if m:
                if not regs:
                    nloads, at = nloads + 1, k
                regs |= named(m.group(1))
            elif code.startswith("s_waitcnt") and "vmcnt" in code:
                regs = set()
        elif regs and named(code) & regs:
            found.append((at, code))
    return found, nloads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("kernel")
    ap.add_argument("--stamps", nargs="*", default=[], help="outputs of tests/diag_stamps.py --out")
    ap.add_argument("--near", type=int, default=8, help="a wait at most this many instructions behind its load is 'near'")
    ap.add_argument("--json", default=None)
    ap.add_argument("--audit", action="store_true", help="only check the asm loads' destinations between issue and wait")
    a = ap.parse_args()
    if a.audit:
        found, nloads = audit(open(a.asm).read(), a.kernel)
        print(f"{a.kernel}: {nloads} asm load statements, {len(found)} instructions naming a destination in flight")
        for at, code in found:
            print(f"  after the statement at line +{at}: {code}")
        raise SystemExit(1 if found or not nloads else 0)
    assert len(PHASES) == NSTAMP
    rows = segment_rows(instructions(open(a.asm).read(), a.kernel))
    stamps = {p: json.load(open(p)) for p in a.stamps}
    print(f"{a.kernel}")
    head = f"{'segment ends at':18s} {'instr':>6s} {'valu':>5s} | " + " ".join(f"{c + ' ld/wt/near':>20s}" for c in CLASSES)
    for p in stamps:
        head += f" | {'cycles':>8s} {'-4 x instr':>10s}"
    print(head)
    for r in rows:
        line = f"{r['ends_at']:18s} {r['instructions']:6d} {r['valu']:5d} | "
        line += " ".join(f"{r['loads'][c]:10d}/{len(r['waits'][c]):3d}/{sum(1 for d in r['waits'][c] if d <= a.near):3d}  "
                         for c in CLASSES)
        r["cycles_per_call"], r["cycles_minus_4_instr"] = {}, {}
        for p, st in stamps.items():
            cyc = st["cycles_per_call"].get(STAMP_KEYS.get(r["ends_at"], r["ends_at"]))
            wait = None if cyc is None or r["ends_at"] not in STRAIGHT else cyc - 4 * r["instructions"]
            r["cycles_per_call"][p], r["cycles_minus_4_instr"][p] = cyc, wait
            line += f" | {'' if cyc is None else int(cyc):>8} {'' if wait is None else int(wait):>10}"
        print(line)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"kernel": a.kernel, "near": a.near, "note": "waits: distance in instructions from the youngest load "
                       "of the class; cycles_minus_4_instr: straight-line phases only", "segments": rows}, f, indent=1)


if __name__ == "__main__":
    main()
