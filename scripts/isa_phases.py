"""Phase-level instruction mix of one kernel in the .s of a -DZB_STAMPS build (static counts per
segment between consecutive phase stamps, in text order). Diagnostic for where the once-per-substep
phases of the step kernel spend their instructions; scripts/isa_loops.py does the same per loop.

    hipcc <product flags> -DZB_STAMPS -DZB_XG_MASK=0x01 --cuda-device-only -S -o stamps.s zb_engine.hip
    python scripts/isa_phases.py stamps.s <kernel symbol> [--json OUT]

A stamp is the `s_memtime` of zb_stamp(); the slot it closes is read from the two LDS offsets of the
read that follows it (stamp[i] and stamp_last, NSTAMP - i slots apart). A segment is named after the stamp
that ends it, which is the phase it covers only where the code between two stamps is straight-line:
the short smooth phases. Segments that the compiler's block placement mixes (the constraint phase,
the solver loops) are printed but say little. Classes are by opcode prefix only.
"""
import json
import re
import sys

PHASES = ["feetech", "kinematics", "com_crb_M", "factor_M", "rne_bias", "solve_smooth", "constraints",
          "nw_warmstart", "nw_update0", "nw_hessian0", "nw_solve0", "line_search", "update_constraint",
          "hessian_refactor", "newton_solve", "newton_check", "sensors", "integrate", "step_end", "forward_entry"]
NSTAMP = len(PHASES)

FP = ("v_add_f", "v_sub_f", "v_subrev_f", "v_mul_f", "v_mul_legacy_f", "v_fma_f", "v_fmac_f", "v_mac_f", "v_mad_f",
      "v_rcp_", "v_rsq_", "v_sqrt_", "v_max_f", "v_min_f", "v_max3_f", "v_min3_f", "v_med3_f", "v_exp_", "v_log_",
      "v_sin_", "v_cos_", "v_fract_", "v_floor_", "v_ceil_", "v_rndne_", "v_trunc_", "v_ldexp_", "v_frexp_",
      "v_cvt_", "v_pk_", "v_div_", "v_mfma_", "v_dot")
SEL = ("v_cndmask", "v_cmp", "v_cmpx")
MOV = ("v_mov_", "v_accvgpr_", "v_swap_")
LANE = ("v_readlane", "v_writelane", "v_readfirstlane")
PERM = ("v_permlane",)
CLASSES = ["fp", "sel_cmp", "move", "integer", "dpp_perm", "lane_rw", "lds", "bpermute", "salu", "vmem", "nop_wait"]


def classify(ins: str) -> str:
    op = ins.split()[0]
    if op.startswith("ds_bpermute") or op.startswith("ds_permute"):
        return "bpermute"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("s_nop", "s_waitcnt")):
        return "nop_wait"
    if op.startswith("s_"):
        return "salu"
    if op.startswith(("global_", "buffer_", "scratch_", "flat_")):
        return "vmem"
    if not op.startswith("v_"):
        return "salu"
    if op.startswith(LANE):
        return "lane_rw"
    if op.startswith(PERM) or "_dpp" in op or " row_" in ins or "quad_perm" in ins or "row_bcast" in ins:
        return "dpp_perm"
    if op.startswith(SEL):
        return "sel_cmp"
    if op.startswith(MOV):
        return "move"
    if op.startswith(FP):
        return "fp"
    return "integer"


def stamp_slot(lines, k):
    """The slot of the stamp at lines[k]: the lane-0 block after it reads stamp[i] and stamp_last
    (= stamp + NSTAMP) with one ds_read2_b64, whose two 8-byte offsets are NSTAMP - i apart."""
    for l in lines[k + 1:k + 16]:
        m = re.match(r"ds_read2_b64 \S+ \S+(?: offset0:(\d+))?(?: offset1:(\d+))?", l)
        if m:
            slot = NSTAMP - (int(m.group(2) or 0) - int(m.group(1) or 0))
            return slot if 0 <= slot < NSTAMP else None
    return None


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
    if out in args:
        args.remove(out)
    s = open(args[0]).read()
    name = args[1]
    i = s.find(name + ":")
    assert i >= 0, f"no symbol {name}"
    j = s.find(".Lfunc_end", i)
    ins = []
    for raw in s[i:j].split("\n")[1:]:
        l = raw.split(";")[0].strip()
        if not l or l.endswith(":") or l.startswith("."):
            continue
        ins.append(l)
    stamps = [k for k, l in enumerate(ins) if l.startswith("s_memtime")]
    slots = [stamp_slot(ins, k) for k in stamps]
    rows = []
    print(f"{name}: {len(ins)} instructions, {len(stamps)} stamps")
    print(f"{'segment ends at':24s} {'len':>6s} {'valu':>6s} " + " ".join(f"{c:>8s}" for c in CLASSES))
    prev = 0
    for k, slot in zip(stamps, slots):
        label = PHASES[slot] if slot is not None else "?"
        seg = ins[prev:k]
        cnt = {c: 0 for c in CLASSES}
        for x in seg:
            cnt[classify(x)] += 1
        valu = sum(1 for x in seg if x.startswith("v_"))
        rows.append({"ends_at": label, "first": prev, "len": len(seg), "valu": valu, **cnt})
        print(f"{label:24s} {len(seg):6d} {valu:6d} " + " ".join(f"{cnt[c]:8d}" for c in CLASSES))
        prev = k
    if out:
        with open(out, "w") as f:
            json.dump({"kernel": name, "instructions": len(ins), "segments": rows}, f, indent=1)


if __name__ == "__main__":
    main()
