"""Lane reads and register moves per phase of the CG headline kernel, and the line search's exit path.

    hipcc <product flags> -DZB_STAMPS -DZB_XG_MASK=0x01 --cuda-device-only -S -o stamps.s zb_engine.hip
    hipcc <product flags>             -DZB_XG_MASK=0x01 --cuda-device-only -S -o unit_a.s zb_engine.hip
    python scripts/spill_census.py --stamps stamps.s --isa unit_a.s [--counts profiles/exec_counts_c2.json]
                                   [--pmc pmc.json --pmc-key cg_8192] [--out profiles/spill_census_c2.json]

Beside scripts/exec_slots.py, which gives the once-per-substep phases as a remainder only. Two things
it does not weigh:

  1. the reloads of spilled scalar registers. The register allocator keeps spilled SGPRs in lanes of
     VGPRs (v_writelane) and reads them back where they are used (v_readlane). Per segment between the
     phase stamps of the -DZB_STAMPS build (scripts/phase_waits.py's cuts), in text order: v_readlane,
     v_writelane, v_readfirstlane and v_mov, and every v_readlane by what first reads the scalar it
     restores: `mask` (a v_cndmask, a 64-bit s_and / s_or / s_andn2 / s_xor / s_cselect, exec, vcc, a
     branch on it), `address` (a load, store or LDS access, or scalar address arithmetic) or `bound`
     (a scalar compare: a loop bound or a uniform test); `other` is what is left (a copy, a VALU
     operand). A pair of reads that rebuilds one 64-bit mask counts as two reads.
     The straight-line phases run once per substep, so their static counts are weighed by the
     substeps of a control step (20 in the headline configuration); a phase that holds divergent
     regions is over-counted by what a whole wave skips.

  2. the line search's exit. From the product build's text (--isa): the instructions between the last
     evaluation's arithmetic and the end of the loop that only restore exec (s_or_b64 exec, exec, ..)
     or copy a register (v_mov_b32 vA, vB), weighed by the line searches of a control step
     (exec_counts.py's `ls`), and the instructions per unrolled evaluation level, weighed by the levels
     a wave runs (`eval_wave`).

--pmc: pmc_summary-style JSON of a counter pass of its own (SQ_INSTS_VALU, SQ_INSTS_SALU, SQ_INSTS,
SQ_INSTS_BRANCH, SQ_ACTIVE_INST_MISC per wave and control step), set beside the census.
The text alone is read; nothing is searched for in it beyond the opcodes named above.
"""
import argparse
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from exec_counts import cg_loop_static, kernel_ins  # noqa: E402
from isa_phases import PHASES, stamp_slot  # noqa: E402
from phase_waits import STRAIGHT, instructions  # noqa: E402

KERNEL = "_ZN2zb11step_kernelILi1ELi0ELi0ELb1ELb0EEEvNS_8StepArgsE"
MASK_OPS = ("s_and_b64", "s_or_b64", "s_xor_b64", "s_andn2_b64", "s_orn2_b64", "s_cselect_b64", "s_not_b64",
            "s_and_saveexec_b64", "s_or_saveexec_b64", "s_andn2_saveexec_b64", "s_mov_b64", "s_cmp_lg_u64", "s_cmp_eq_u64")
MEM = ("s_load", "s_buffer_load", "global_", "buffer_", "flat_", "scratch_", "ds_")
ADDR_OPS = ("s_add_u32", "s_addc_u32", "s_add_i32", "s_sub_u32", "s_subb_u32", "s_lshl_b32", "s_lshl_b64", "s_mul_i32",
            "s_lshl1_add_u32", "s_lshl2_add_u32", "s_lshl3_add_u32", "s_lshl4_add_u32", "s_ashr_i32")
LOOK = 400  # instructions to look ahead for a restored scalar's first reader


def sregs(tok):
    """The scalar registers an operand names: s5 -> {5}, s[4:5] -> {4, 5}."""
    out = set()
    for lo, hi in re.findall(r"\bs\[(\d+):(\d+)\]", tok):
        out |= set(range(int(lo), int(hi) + 1))
    out |= {int(r) for r in re.findall(r"\bs(\d+)\b", tok)}
    return out


def consumer(ins, k):
    """Class of the first instruction after ins[k] (a v_readlane) that reads its scalar destination."""
    dst = int(re.match(r"v_readlane_b32 s(\d+),", ins[k]).group(1))
    for x in ins[k + 1:k + 1 + LOOK]:
        op = x.split()[0]
        ops = x[len(op):].split(",")
        reads = ops[1:] if len(ops) > 1 and not op.startswith(("s_cmp", "s_cbranch", "s_bitcmp")) else ops
        if op.startswith(("global_store", "buffer_store", "flat_store", "scratch_store", "ds_write")):
            reads = ops
        if dst in sregs(",".join(reads)):
            if op.startswith("v_cndmask") or op.startswith(MASK_OPS) or op.startswith("s_cbranch"):
                return "mask"
            if op.startswith(MEM) or op.startswith(ADDR_OPS):
                return "address"
            if op.startswith(("s_cmp", "s_bitcmp")):
                return "bound"
            return "other"
        if dst in sregs(ops[0]) and not op.startswith(("s_cmp", "s_cbranch")):
            return "other"  # overwritten before any read in text order (the reader sits on another path)
    return "other"


def lane_census(ins, lo, hi):
    row = {"instructions": hi - lo, "v_readlane": 0, "v_writelane": 0, "v_readfirstlane": 0, "v_mov": 0,
           "readlane_by_consumer": {"mask": 0, "address": 0, "bound": 0, "other": 0}}
    for k in range(lo, hi):
        op = ins[k].split()[0]
        if op == "v_readlane_b32":
            row["v_readlane"] += 1
            row["readlane_by_consumer"][consumer(ins, k)] += 1
        elif op == "v_writelane_b32":
            row["v_writelane"] += 1
        elif op == "v_readfirstlane_b32":
            row["v_readfirstlane"] += 1
        elif op.startswith("v_mov_b32"):
            row["v_mov"] += 1
    return row


def phases(stamps_asm, kernel, substeps):
    ins = instructions(open(stamps_asm).read(), kernel)
    cuts = [k for k, l in enumerate(ins) if l.startswith("s_memtime")]
    rows, prev = [], 0
    for k in cuts + [len(ins)]:
        slot = stamp_slot(ins, k) if k < len(ins) else None
        name = PHASES[slot] if slot is not None else ("(after the last stamp)" if k == len(ins) else "?")
        r = lane_census(ins, prev, k)
        r["ends_at"] = name
        r["straight_line"] = name in STRAIGHT
        if r["straight_line"]:
            r["executed_per_control_step"] = {c: r[c] * substeps for c in ("v_readlane", "v_writelane", "v_readfirstlane", "v_mov")}
            r["executed_per_control_step"]["readlane_mask"] = r["readlane_by_consumer"]["mask"] * substeps
        rows.append(r)
        prev = k
    return rows, len(ins)


def ladder(isa, kernel):
    """The CG loop's line search in the product text: instructions per evaluation level (the copy
    without the limit row) and the exit path behind the last level."""
    ins, _ = kernel_ins(isa, kernel)
    lo, hi = cg_loop_static(isa, kernel)["loop"]
    med = [k for k in range(lo, hi + 1) if ins[k].startswith("v_med3_f32")]
    half = max(range(1, len(med)), key=lambda i: med[i] - med[i - 1])
    nolim = med[:half]
    per_level = (nolim[-1] - nolim[0]) / (len(nolim) - 1)
    # behind the last level of the copy: the run of exec restores and copies before the next arithmetic
    k = nolim[-1]
    tail = ins[k:med[half]]
    restores = [x for x in tail if re.match(r"s_or_b64 exec, exec, ", x)]
    copies = [x for x in tail if re.match(r"v_mov_b32_e32 v\d+, v\d+$", x)]
    run, best = 0, 0
    for x in tail:
        if re.match(r"s_or_b64 exec, exec, ", x) or re.match(r"v_mov_b32_e32 v\d+, v\d+$", x):
            run += 1
            best = max(best, run)
        else:
            run = 0
    return {"levels": len(nolim), "instructions_per_level": round(per_level, 1),
            "exec_restores_behind_last_level": len(restores), "register_copies_behind_last_level": len(copies),
            "longest_run_of_restores_and_copies": best, "kernel_instructions": len(ins), "cg_loop": [lo, hi],
            "lane_rw_in_cg_loop": lane_census(ins, lo, hi + 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stamps", required=True, help="assembly of the -DZB_STAMPS build of the first unit")
    ap.add_argument("--isa", required=True, help="assembly of the product build of the first unit")
    ap.add_argument("--kernel", default=KERNEL)
    ap.add_argument("--substeps", type=int, default=20)
    ap.add_argument("--counts", default="", help="exec_counts.py's JSON")
    ap.add_argument("--pmc", default="", help="JSON with per-wave counters of a counter pass")
    ap.add_argument("--pmc-key", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rows, n = phases(a.stamps, a.kernel, a.substeps)
    lad = ladder(a.isa, a.kernel)
    res = {"kernel": a.kernel, "stamps_build_instructions": n, "substeps_per_control_step": a.substeps, "phases": rows,
           "line_search": lad}
    straight = [r for r in rows if r["straight_line"]]
    tot = {c: sum(r["executed_per_control_step"][c] for r in straight) for c in ("v_readlane", "readlane_mask", "v_mov", "v_writelane", "v_readfirstlane")}
    res["straight_line_phases_executed_per_control_step"] = tot
    if a.counts:
        per = json.load(open(a.counts))["per_env_step"]
        ex = {"line_searches": per["ls"], "levels_run_by_the_wave": per["eval_wave"]}
        ex["level_slots"] = round(lad["instructions_per_level"] * per["eval_wave"])
        ex["exit_path_slots (longest run of restores and copies x line searches)"] = round(lad["longest_run_of_restores_and_copies"] * per["ls"])
        res["line_search_executed_per_control_step"] = ex
    if a.pmc:
        p = json.load(open(a.pmc))
        for k in [x for x in a.pmc_key.split("/") if x]:
            p = p[k]
        res["pmc_per_wave"] = p
    print(f"{'segment ends at':24s} {'instr':>6s} {'rdlane':>6s} {'mask':>5s} {'addr':>5s} {'bound':>5s} {'other':>5s} {'wrlane':>6s} {'rdfirst':>7s} {'v_mov':>6s}  straight")
    for r in rows:
        c = r["readlane_by_consumer"]
        print(f"{r['ends_at']:24s} {r['instructions']:6d} {r['v_readlane']:6d} {c['mask']:5d} {c['address']:5d} {c['bound']:5d} {c['other']:5d} "
              f"{r['v_writelane']:6d} {r['v_readfirstlane']:7d} {r['v_mov']:6d}  {'x' + str(a.substeps) if r['straight_line'] else ''}")
    print("straight-line phases, executed per control step:", tot)
    print("line search:", {k: v for k, v in lad.items() if k != "lane_rw_in_cg_loop"})
    if a.counts:
        print("line search, executed per control step:", res["line_search_executed_per_control_step"])
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
