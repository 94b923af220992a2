"""Memory loads and the waits on them, per loop of one kernel in a hipcc -S / --save-temps .s file.

    python scripts/isa_waits.py <file.s> <kernel symbol> [--waits all|loops|none] [--max-dist N]

Beside isa_loops.py (instruction mix per back edge) and isa_phases.py. Static, from the compiler's
own loop annotations ("Loop Header: Depth=", "in Loop: Header=", "Parent Loop"):

  - per loop, the scalar-memory loads (s_load / s_buffer_load), global loads (global / flat /
    buffer), scratch loads and LDS operations (ds_*) in its own blocks and with its child loops;
  - for every s_waitcnt, the counter it drains (vmcnt: vector memory; lgkmcnt: scalar memory and
    LDS) and how many instructions were issued since the youngest load of that class in program
    order. A small distance is a load the wave sits out almost in full: nothing but the other wave
    of the SIMD covers it.

Distances follow the text's order, so across a branch they are an estimate; within a block they are
exact. On gfx9 a store counts in vmcnt as well; only loads are tracked as the thing waited for.
"""
import argparse
import re
import sys

CLASSES = ("smem", "global", "scratch", "lds")


def classify(op):
    if op.startswith(("s_load_", "s_buffer_load_")):
        return "smem"
    if op.startswith("scratch_load_"):
        return "scratch"
    if op.startswith(("global_load_", "flat_load_", "buffer_load_")):
        return "global"
    if op.startswith("ds_"):
        return "lds"
    return None


def parse(text, name):
    i = text.find("\n" + name + ":")
    if i < 0:
        sys.exit(f"kernel {name} not found")
    j = text.find(".Lfunc_end", i)
    ins = []      # (op, full line, innermost loop header or None)
    parents = {}  # loop header -> parent header or None
    depth = {}
    cur = None    # innermost loop of the current block
    label = None
    pending = []  # the annotation lines of the block being opened
    def close_block():
        nonlocal cur
        if label is None:
            return
        txt = " ".join(pending)
        m = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", txt)
        if m:
            cur = label
            depth[label] = int(m.group(1))
            ps = re.findall(r"Parent Loop (\S+) Depth=(\d+)", txt)
            parents[label] = max(ps, key=lambda p: int(p[1]))[0] if ps else None
        else:
            m = re.search(r"in Loop: Header=(\S+) Depth=(\d+)", txt)
            cur = m.group(1) if m else None
    opened = True
    for raw in text[i:j].split("\n")[2:]:
        code, _, comment = raw.partition(";")
        code = code.strip()
        m = re.match(r"\.?(L?BB\d+_\d+):", code)
        if m:
            label, pending, opened = m.group(1).lstrip("L"), [comment], False
            continue
        if not code:
            if not opened:
                pending.append(comment)
            continue
        if code.startswith(".") or code.endswith(":"):
            continue
        if not opened:
            close_block()
            opened = True
        ins.append((code.split()[0], code, cur))
    return ins, parents, depth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("kernel")
    ap.add_argument("--waits", default="all", choices=["all", "loops", "none"],
                    help="list every s_waitcnt, those inside loops only, or none (the tables alone)")
    ap.add_argument("--max-dist", type=int, default=None, help="list only waits at most this far from their load")
    a = ap.parse_args()
    ins, parents, depth = parse(open(a.asm).read(), a.kernel)

    def chain(h):
        out = []
        while h is not None:
            out.append(h)
            h = parents.get(h)
        return out

    own = {h: dict.fromkeys(CLASSES + ("n",), 0) for h in parents}
    incl = {h: dict.fromkeys(CLASSES + ("n",), 0) for h in parents}
    total = dict.fromkeys(CLASSES + ("n",), 0)
    for op, _, h in ins:
        c = classify(op)
        for k in filter(None, (c, "n")):
            total[k] += 1
            if h in own:
                own[h][k] += 1
            for p in chain(h):
                if p in incl:
                    incl[p][k] += 1
    print(f"{a.kernel}: {len(ins)} instructions, {len(parents)} loops; loads in the whole kernel: "
          + ", ".join(f"{k} {total[k]}" for k in CLASSES))
    print("loop         depth parent       instr(own/incl)  smem(own/incl) global(own/incl) scratch(own/incl) lds(own/incl)")
    order = {}
    for k, (_, _, h) in enumerate(ins):
        order.setdefault(h, k)
    for h in sorted(parents, key=lambda x: order.get(x, 1 << 30)):
        o, t = own[h], incl[h]
        print(f"{h:12s} {depth[h]:5d} {str(parents[h] or '-'):12s} {o['n']:7d}/{t['n']:<7d} "
              + " ".join(f"{o[k]:8d}/{t[k]:<6d}" for k in CLASSES))

    # the waits: distance from the youngest load of the class the counter covers
    last = dict.fromkeys(CLASSES, None)
    rows = []
    for k, (op, line, h) in enumerate(ins):
        c = classify(op)
        if c:
            last[c] = k
        if op != "s_waitcnt":
            continue
        for cnt, classes in (("vmcnt", ("global", "scratch")), ("lgkmcnt", ("smem", "lds"))):
            m = re.search(cnt + r"\((\d+)\)", line)
            if not m:
                continue
            young = [(last[x], x) for x in classes if last[x] is not None]
            if not young:
                rows.append((k, h, cnt, int(m.group(1)), None, "-"))
                continue
            at, what = max(young)
            rows.append((k, h, cnt, int(m.group(1)), k - at - 1, what))
    if a.waits != "none":
        print("\nwaits: index  loop          counter(left)  youngest load  instructions since it")
        for k, h, cnt, left, d, what in rows:
            if a.waits == "loops" and h is None:
                continue
            if a.max_dist is not None and (d is None or d > a.max_dist):
                continue
            print(f"  {k:6d}  {str(h or '-'):12s}  {cnt:8s}({left:2d})  {what:8s}  {'' if d is None else d}")
    # summary: how close the waits sit to their loads
    print("\nwaits by class of the youngest load: count, and how many within 4 / 8 / 16 / 32 instructions of it")
    for what in CLASSES:
        ds = [d for _, _, _, _, d, w in rows if w == what and d is not None]
        print(f"  {what:8s} {len(ds):4d}   " + "  ".join(f"<={b}: {sum(1 for d in ds if d <= b)}" for b in (4, 8, 16, 32)))


if __name__ == "__main__":
    main()
