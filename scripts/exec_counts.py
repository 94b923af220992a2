"""Executed counts of the CG headline kernel's solver blocks, and from them executed VALU per phase.

    make -C ksim-gym-zbot_amd/csrc blockcount
    python scripts/exec_counts.py [--n 8192 --steps 6] [--isa unit_a.s] [--pmc-valu 109200] [--out counts.json]

The -DZB_STAMPS -DZB_BLOCKCOUNT build (csrc/Makefile `blockcount`) keeps counters in the stamp
slots instead of phase times: forward() passes, CG solves, line searches (entered, returned at the
slope / curvature test, run in the joint-limit copy), evaluations per team and per wave (a wave
runs the larger of its two teams' counts), how each CG iteration ended (the cap, the tolerance, a
further iteration), and the cycles of the prologue (make_ctx, load_state, load_params) and the
epilogue (the state store). This script runs the C2 workload on that build and prints the counts
per env and control step.

With --isa (the assembly of the product's first unit, `hipcc <product flags> -DZB_XG_MASK=0x01
--cuda-device-only -S`) it also weighs the static VALU of the CG iteration loop's blocks by those
counts: the loop is one natural loop without children whose evaluation bodies each hold one
v_med3_f32 (the friction-loss clamp), so the text between two of them is one evaluation plus the
bracket update before it, and what precedes the first and follows the last copy is the iteration's
fixed part (mul_m_dot and the line-search setup before, update_constraint_lane, solve_pre and the
four-sum after). The remainder against --pmc-valu (SQ_INSTS_VALU per wave of an unmodified build,
scripts/pmc_latency.sh) is what runs outside the CG iteration loop: the once-per-substep phases
and the step end.
"""
import argparse
import ctypes as C
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ksim-gym-zbot_amd"))

NAMES = ["forward", "solve", "ls", "ls_ret0", "ls_limit", "eval", "eval_wave", "it_cap", "it_tol", "it_full",
         "prologue_cyc", "epilogue_cyc", "step"]
KERNEL = "_ZN2zb11step_kernelILi1ELi0ELi0ELb1ELb0EEEvNS_8StepArgsE"
NSLOTS = 20


def kernel_ins(path, name):
    s = open(path).read()
    i = s.find(name + ":")
    assert i >= 0, f"no symbol {name}"
    j = s.find(".Lfunc_end", i)
    labels, ins = {}, []
    for raw in s[i:j].split("\n")[1:]:
        l = raw.split(";")[0].strip()
        if not l or l.startswith("."):
            if l.endswith(":"):
                labels[l[:-1]] = len(ins)
            continue
        if l.endswith(":"):
            labels[l[:-1]] = len(ins)
            continue
        ins.append(l)
    return ins, labels


def cg_loop_static(path, name=KERNEL):
    """Static VALU of the CG iteration loop's parts: (fixed before, per evaluation [no-limit copy],
    per evaluation [limit copy], fixed after), from the loop that holds the evaluations' v_med3_f32."""
    ins, labels = kernel_ins(path, name)
    med = [k for k, l in enumerate(ins) if l.startswith("v_med3_f32")]
    loops = []
    for k, l in enumerate(ins):
        m = re.match(r"s_(cbranch_\w+|branch)\s+(\S+)", l)
        if m and m.group(2) in labels and labels[m.group(2)] <= k:
            loops.append((labels[m.group(2)], k))
    inner = [(a, b) for a, b in loops if sum(a <= k <= b for k in med) >= 12]
    # the compiler nests the iteration's exits as loops of their own around the evaluations: the
    # iteration is the largest of the loops that are not much longer than the smallest
    short = min(b - a for a, b in inner)
    a, b = max((ab for ab in inner if ab[1] - ab[0] <= 2 * short), key=lambda ab: ab[1] - ab[0])
    med = [k for k in med if a <= k <= b]
    valu = lambda lo, hi: sum(1 for l in ins[lo:hi] if l.startswith("v_"))
    # the two copies (without and with the joint-limit row) are the two runs of evenly spaced clamps
    half = max(range(1, len(med)), key=lambda i: med[i] - med[i - 1])
    # an evaluation starts at the two fmas before its clamp; cut at the clamps themselves (the offset
    # is the same for every copy)
    per_nolim = valu(med[0], med[half - 1]) / (half - 1)
    per_lim = valu(med[half], med[-1]) / (len(med) - half - 1)
    before = valu(a, med[0])
    after = valu(med[-1], b + 1) - per_lim
    return {"loop": [a, b], "evaluation_copies": len(med), "valu_loop": valu(a, b + 1), "valu_before_first_eval": before,
            "valu_per_eval_nolimit": round(per_nolim, 1), "valu_per_eval_limit": round(per_lim, 1),
            "valu_after_last_eval": round(after, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--lib", default="libzbot_hip_blockcount.so")
    ap.add_argument("--isa", default="")
    ap.add_argument("--pmc-valu", type=float, default=0.0, help="SQ_INSTS_VALU per wave of the unmodified build")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    res = {}
    if a.isa:
        res["static"] = cg_loop_static(a.isa)
    import torch  # noqa: PLC0415
    from zbot_amd import compile_model, default_config  # noqa: PLC0415
    from zbot_amd.engine import HipEngine  # noqa: PLC0415

    cm = compile_model()
    eng = HipEngine(cm, default_config(solver="cg"), a.n, seed=1, lib_path=os.path.join(ROOT, "ksim-gym-zbot_amd", "zbot_amd", a.lib))
    eng.L.zb_get_stamps.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    eng.reset()
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    bias = torch.tensor([cm.cmodel.joint_bias[i] for i in range(20)], device="cuda")
    tot = torch.zeros(NSLOTS, dtype=torch.float64)
    for _ in range(a.steps):
        eng.step(bias + 0.05 * torch.randn(a.n, 20, device="cuda", generator=g), extras=False)
        buf = torch.zeros(a.n, NSLOTS, dtype=torch.int64, device="cuda")
        eng.L.zb_get_stamps(eng.h, buf.data_ptr(), eng._stream())
        torch.cuda.synchronize()
        tot += buf.cpu().double().sum(0)
    per = {k: float(tot[i]) / (a.n * a.steps) for i, k in enumerate(NAMES)}
    res["per_env_step"] = {k: round(v, 3) for k, v in per.items()}
    ls = max(per["ls"] - per["ls_ret0"], 1e-9)
    res["trip_counts"] = {
        "cg_iterations_per_substep": round(per["ls"] / max(per["forward"], 1e-9), 3),
        "evaluations_per_line_search_per_env": round(per["eval"] / ls, 3),
        "evaluations_per_line_search_per_wave": round(per["eval_wave"] / ls, 3),
        "line_searches_in_limit_copy_frac": round(per["ls_limit"] / max(per["ls"], 1e-9), 4),
        "line_searches_returned_at_entry_frac": round(per["ls_ret0"] / max(per["ls"], 1e-9), 4),
        "iterations_ended_by_cap_frac": round(per["it_cap"] / max(per["ls"], 1e-9), 4),
        "iterations_ended_by_tolerance_frac": round(per["it_tol"] / max(per["ls"], 1e-9), 4),
    }
    if a.isa:
        st = res["static"]
        # a wave runs an iteration while either team is in it: the per-wave counts are bounded below by
        # the per-env ones and above by twice them; the evaluations' wave count is measured, the
        # iteration's is taken as the per-env count (both teams of a wave run nearly the same number)
        lim = res["trip_counts"]["line_searches_in_limit_copy_frac"]
        per_eval = lim * st["valu_per_eval_limit"] + (1 - lim) * st["valu_per_eval_nolimit"]
        ex = {
            "cg_loop_before_evals (mul_m_dot, line-search setup)": per["ls"] * st["valu_before_first_eval"],
            "cg_loop_evaluations": per["eval_wave"] * per_eval,
            "cg_loop_after_evals (update_constraint_lane, solve_pre, four-sum)":
                (per["it_full"] + per["it_tol"]) * st["valu_after_last_eval"],
        }
        ex["cg_loop_total"] = sum(ex.values())
        if a.pmc_valu:
            ex["outside_cg_loop (once-per-substep phases, warm start, step end) = PMC - loop"] = a.pmc_valu - ex["cg_loop_total"]
            ex["pmc_insts_valu_per_wave"] = a.pmc_valu
        res["executed_valu_per_wave_and_control_step"] = {k: round(v) for k, v in ex.items()}
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
