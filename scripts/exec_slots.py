"""Issue-slot census of the CG headline kernel: every instruction class, not VALU alone.

    python scripts/exec_slots.py --isa unit_a.s [--counts profiles/exec_counts_c2.json]
                                 [--pmc pmc_memops.json --pmc-key parent/cg_512] [--out census.json]

scripts/exec_counts.py weighs the static VALU of the CG iteration loop's parts by the executed block
counts of the -DZB_BLOCKCOUNT build. This script does the same for every class of instruction that
takes an issue slot of the wave, from the assembly of the product's first unit (`hipcc <product
flags> -DZB_XG_MASK=0x01 --cuda-device-only -S`) and the trip counts that exec_counts.py wrote
(`per_env_step` of its JSON; the counts depend on the states alone, so a build that keeps every bit
keeps them):

  VALU as scripts/isa_phases.py splits it (fp, sel_cmp, move, integer, dpp_perm); lane_rw
  (v_readlane / v_writelane / v_readfirstlane); LDS (with ds_bpermute); vector memory;
  SALU split into exec-mask operations (anything that writes exec: *_saveexec, s_or/and/andn2 ...
  exec), lane-mask logic (64-bit s_and/or/xor/andn2/orn2/cselect/not on SGPR pairs), scalar memory
  and the rest (moves, compares, address work); s_nop (instructions and wait states); s_waitcnt;
  branches.

The CG iteration loop is cut as exec_counts.py cuts it (before the evaluations, per evaluation,
after them) and each part's static counts are weighed by ls, eval_wave and it_full + it_tol. What
runs outside the loop (the once-per-substep phases, the warm start, the step end) is given as static
text only, and, with --pmc (scripts/pmc_memops.sh, a counter pass of its own), as the remainder of
the executed VALU / SALU / LDS per wave. SQ_INSTS_SALU holds neither s_nop, s_waitcnt nor branches
(the loop's alone would exceed it); with SQ_INSTS_BRANCH and SQ_INSTS in the pass those are checked too.
Divergent regions inside a part are counted as executed whenever the part is, which is what a wave
with lanes on both sides of a predicate does; a region that a whole wave skips (the joint-limit row,
the empty bank) is over-counted by that much.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from exec_counts import cg_loop_static, kernel_ins  # noqa: E402
from isa_phases import classify as phase_class  # noqa: E402

KERNEL = "_ZN2zb11step_kernelILi1ELi0ELi0ELb1ELb0EEEvNS_8StepArgsE"
CLASSES = ["fp", "sel_cmp", "move", "integer", "dpp_perm", "lane_rw", "lds", "vmem", "salu_exec", "salu_lanemask",
           "salu_smem", "salu_other", "s_nop", "s_waitcnt", "branch"]
MASK_OPS = ("s_and_b64", "s_or_b64", "s_xor_b64", "s_andn2_b64", "s_orn2_b64", "s_nand_b64", "s_nor_b64", "s_xnor_b64",
            "s_not_b64", "s_cselect_b64")


def classify(ins: str) -> str:
    op = ins.split()[0]
    if op == "s_nop":
        return "s_nop"
    if op == "s_waitcnt":
        return "s_waitcnt"
    if op.startswith(("s_cbranch", "s_branch", "s_setpc", "s_swappc", "s_call", "s_endpgm")):
        return "branch"
    if op.startswith(("s_load", "s_buffer_load", "s_memtime", "s_memrealtime")):
        return "salu_smem"
    if op.startswith("s_"):
        dst = ins[len(op):].split(",")[0].strip()
        if "saveexec" in op or dst.startswith("exec"):
            return "salu_exec"
        if op.startswith(MASK_OPS):
            return "salu_lanemask"
        return "salu_other"
    c = phase_class(ins)
    return {"bpermute": "lds", "salu": "salu_other", "nop_wait": "s_nop"}.get(c, c)


def census(seg):
    cnt = {c: 0 for c in CLASSES}
    ws = 0
    for x in seg:
        cnt[classify(x)] += 1
        if x.startswith("s_nop"):
            ws += int(x.split()[1], 0) + 1
    cnt["nop_wait_states"] = ws
    cnt["all"] = len(seg)
    return cnt


def scaled(c, w):
    return {k: round(v * w, 1) for k, v in c.items()}


def add(a, b):
    return {k: round(a[k] + b[k], 1) for k in a}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--isa", required=True)
    ap.add_argument("--kernel", default=KERNEL)
    ap.add_argument("--counts", default="", help="exec_counts.py's JSON (per_env_step)")
    ap.add_argument("--pmc", default="", help="pmc_memops_summary.py's JSON")
    ap.add_argument("--pmc-key", default="cg_512", help="path of the entry in it, e.g. parent/cg_512")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ins, _ = kernel_ins(a.isa, a.kernel)
    st = cg_loop_static(a.isa, a.kernel)
    lo, hi = st["loop"]
    med = [k for k in range(lo, hi + 1) if ins[k].startswith("v_med3_f32")]
    half = max(range(1, len(med)), key=lambda i: med[i] - med[i - 1])
    parts = {
        "before_evals": ins[lo:med[0]],
        "evals_nolimit": ins[med[0]:med[half - 1]],
        "evals_limit": ins[med[half]:med[-1]],
    }
    n_nolim, n_lim = half - 1, len(med) - half - 1
    per_lim = scaled(census(parts["evals_limit"]), 1.0 / n_lim)
    tail = census(ins[med[-1]:hi + 1])
    after = {k: round(tail[k] - per_lim[k], 1) for k in tail}
    res = {"kernel": a.kernel, "instructions": len(ins), "static": {
        "kernel": census(ins), "cg_loop": census(ins[lo:hi + 1]), "cg_loop_before_evals": census(parts["before_evals"]),
        "cg_loop_per_eval_nolimit": scaled(census(parts["evals_nolimit"]), 1.0 / n_nolim), "cg_loop_per_eval_limit": per_lim,
        "cg_loop_after_evals": after, "outside_cg_loop": census(ins[:lo] + ins[hi + 1:])}}
    if a.counts:
        per = json.load(open(a.counts))["per_env_step"]
        lim = per["ls_limit"] / max(per["ls"], 1e-9)
        ev = add(scaled(res["static"]["cg_loop_per_eval_limit"], lim * per["eval_wave"]),
                 scaled(res["static"]["cg_loop_per_eval_nolimit"], (1 - lim) * per["eval_wave"]))
        ex = {"cg_loop_before_evals": scaled(res["static"]["cg_loop_before_evals"], per["ls"]), "cg_loop_evaluations": ev,
              "cg_loop_after_evals": scaled(after, per["it_full"] + per["it_tol"])}
        ex["cg_loop_total"] = add(add(ex["cg_loop_before_evals"], ev), ex["cg_loop_after_evals"])
        res["trip_counts"] = {k: per[k] for k in ("ls", "eval_wave", "it_full", "it_tol", "ls_limit")}
        t = ex["cg_loop_total"]
        valu = sum(t[c] for c in ("fp", "sel_cmp", "move", "integer", "dpp_perm", "lane_rw"))
        salu = sum(t[c] for c in ("salu_exec", "salu_lanemask", "salu_other"))
        ex["cg_loop_by_counter"] = {"VALU": round(valu), "SALU": round(salu), "LDS": round(t["lds"]),
                                    "BRANCH": round(t["branch"]), "NOP_WAITCNT": round(t["s_nop"] + t["s_waitcnt"])}
        if a.pmc:
            p = json.load(open(a.pmc))
            for k in a.pmc_key.split("/"):
                p = p[k]
            pw = p["per_wave"]
            ex["pmc_per_wave"] = pw
            rest = {"VALU": round(pw["VALU"] - valu), "SALU": round(pw["SALU"] - salu), "LDS": round(pw["LDS"] - t["lds"])}
            if "BRANCH" in pw:
                rest["BRANCH"] = round(pw["BRANCH"] - t["branch"])
            if "SQ_INSTS" in pw:
                pw = dict(pw, INSTS=pw["SQ_INSTS"])
            if "INSTS" in pw:
                # what no class counter holds: s_nop, s_waitcnt and the other wave-control instructions
                other = pw["INSTS"] - sum(pw.get(c, 0) for c in ("VALU", "SALU", "SMEM", "LDS", "BRANCH", "VMEM_RD", "VMEM_WR"))
                ex["pmc_unclassified (s_nop, s_waitcnt, ...)"] = round(other)
                rest["NOP_WAITCNT"] = round(other - t["s_nop"] - t["s_waitcnt"])
            ex["outside_cg_loop = PMC - loop"] = rest
            tot = pw.get("INSTS") or sum(pw.get(c, 0) for c in ("VALU", "SALU", "SMEM", "LDS", "VMEM_RD", "VMEM_WR"))
            ex["pmc_instructions_per_wave"] = round(tot)
            ex["cg_loop_share_of_pmc_instructions"] = {c: round(t[c] / tot, 4) for c in CLASSES}
        res["executed_per_wave_and_control_step"] = ex
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
