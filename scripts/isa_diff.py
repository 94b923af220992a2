#!/usr/bin/env python3
"""Do two revisions of the step kernel compile to the same instructions?

    scripts/isa_diff.py REV_A [REV_B|cur|FILE] [--json PATH] [--jobs N] [--no-cache]

Builds both compilation units of zb_engine.hip (csrc/Makefile: unit A, the collider sets XG_MASK_A
under ENGINE_SCHED; unit B, XG_MASK_B with -DZB_ENGINE_TU_B) of each revision to gfx950 assembly
(--cuda-device-only -S; no GPU needed) with the Makefile's own flags, drops the lines that contain
__hip_cuid_ (a symbol that hashes the source text) and compares the text kernel by kernel, keyed by
the .amdhsa_kernel name: a kernel's text runs from the end of the kernel before it to its own
.end_amdhsa_kernel, and what follows the last kernel (the metadata) is compared as "(rest)". The
text alone is compared; nothing is searched for in it. `cur` is the working tree, FILE the path of
some other copy of zb_engine.hip (a variant under trial). The headers are
the working tree's for both sides, as in scripts/ab_build.sh.

Prints one line per kernel and writes the SHA-256 of every kernel's text on both sides to PATH.
The assembly (about 15 MB per unit) stays in evariants/isa_diff/, which git ignores; a revision's
files are kept there (a commit's under its hash, the working tree's under the hash of its text) and
reused by the next run with the same flags, compiler version and headers (--no-cache: never).
Exit status 1 if any kernel differs.
"""

import argparse
import hashlib
import json
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ksim-gym-zbot_amd", "csrc")
SRC = "ksim-gym-zbot_amd/csrc/zb_engine.hip"
WORK = os.path.join(ROOT, "evariants", "isa_diff")


def make_vars() -> dict:
    """The Makefile's plain `NAME = value` / `NAME ?= value` assignments, $(NAME) expanded."""
    raw = {}
    for line in open(os.path.join(CSRC, "Makefile")):
        m = re.match(r"^([A-Z_]+) *\??= *(.*)$", line.rstrip("\n"))
        if m:
            raw[m.group(1)] = m.group(2)

    def expand(v):
        return re.sub(r"\$\(([A-Z_]+)\)", lambda m: expand(raw[m.group(1)]), v)

    return {k: expand(v) for k, v in raw.items()}


def unit_flags(mv: dict) -> dict:
    """The two units' flags. The Makefile's include paths are relative to csrc/; a revision is compiled
    from a directory of its own, so they are made absolute, and csrc/ itself is added (zb_internal.h)."""
    def absolute(f):
        return "-I" + os.path.normpath(os.path.join(CSRC, f[2:])) if f.startswith("-I") and not os.path.isabs(f[2:]) else f

    base = [absolute(f) for f in mv["FLAGS"].split()] + ["-I" + CSRC]
    dev = ["--cuda-device-only", "-S"]
    return {
        "A": base + mv["ENGINE_SCHED"].split() + [f"-DZB_XG_MASK={mv['XG_MASK_A']}"] + dev,
        "B": base + ["-DZB_ENGINE_TU_B", f"-DZB_XG_MASK={mv['XG_MASK_B']}"] + dev,
    }


def build_stamp(flags: list, hipcc: str) -> str:
    """What a kept assembly file depends on besides its source: the flags, the compiler, and the
    working tree's headers (used for both sides)."""
    h = hashlib.sha256()
    for d in (CSRC, os.path.join(ROOT, "include")):
        for name in sorted(os.listdir(d)):
            if name.endswith(".h"):
                h.update(name.encode() + open(os.path.join(d, name), "rb").read())
    ver = subprocess.run([hipcc, "--version"], capture_output=True, text=True).stdout
    return " ".join(flags) + "\nheaders " + h.hexdigest() + "\n" + ver


def checkout(rev: str) -> str:
    """A directory that holds the revision's zb_engine.hip under that name: a commit's under its hash,
    the working tree's (`cur`) or a file's under the hash of its text."""
    if rev == "cur" or os.path.isfile(rev):
        text = open(os.path.join(ROOT, SRC) if rev == "cur" else rev, "rb").read()
        d = os.path.join(WORK, "cur-" + hashlib.sha256(text).hexdigest()[:16])
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "zb_engine.hip"), "wb") as f:
            f.write(text)
        return d
    sha = subprocess.run(["git", "-C", ROOT, "rev-parse", "--verify", rev + "^{commit}"], check=True,
                         capture_output=True, text=True).stdout.strip()
    d = os.path.join(WORK, sha)
    os.makedirs(d, exist_ok=True)
    text = subprocess.run(["git", "-C", ROOT, "show", f"{sha}:{SRC}"], check=True, capture_output=True).stdout
    with open(os.path.join(d, "zb_engine.hip"), "wb") as f:
        f.write(text)
    return d


def assemble(d: str, unit: str, flags: list, hipcc: str, fresh: bool) -> str:
    out = os.path.join(d, f"unit_{unit}.s")
    stamp = out + ".stamp"
    line = build_stamp(flags, hipcc)
    if not fresh and os.path.exists(out) and os.path.exists(stamp) and open(stamp).read() == line:
        return out
    # compiled from its own directory under the same relative name on both sides (the assembly names
    # its source)
    cmd = [hipcc] + flags + ["-o", "unit_" + unit + ".s", "zb_engine.hip"]
    subprocess.run(cmd, check=True, cwd=d)
    with open(stamp, "w") as f:
        f.write(line)
    return out


def kernels(path: str) -> dict:
    """{kernel name: sha256 of its text}, "(rest)" for what follows the last kernel."""
    out, chunk, name = {}, hashlib.sha256(), None
    with open(path, errors="replace") as f:
        for line in f:
            if "__hip_cuid_" in line:
                continue
            chunk.update(line.encode())
            s = line.strip()
            if s.startswith(".amdhsa_kernel "):
                name = s.split(None, 1)[1]
            elif s == ".end_amdhsa_kernel":
                assert name is not None and name not in out, (path, name)
                out[name] = chunk.hexdigest()
                chunk, name = hashlib.sha256(), None
    out["(rest)"] = chunk.hexdigest()
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("rev_a")
    ap.add_argument("rev_b", nargs="?", default="cur")
    ap.add_argument("--json", default=None, help="write the per-kernel hashes of both sides here")
    ap.add_argument("--jobs", type=int, default=4, help="compilations at a time (four in all)")
    ap.add_argument("--no-cache", action="store_true", help="compile everything again")
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    a = ap.parse_args()
    flags = unit_flags(make_vars())
    dirs = {rev: checkout(rev) for rev in (a.rev_a, a.rev_b)}
    jobs = [(rev, u) for rev in dirs for u in flags]
    with ThreadPoolExecutor(max(1, a.jobs)) as ex:
        paths = list(ex.map(lambda j: assemble(dirs[j[0]], j[1], flags[j[1]], a.hipcc, a.no_cache), jobs))
    hashes = {j: kernels(p) for j, p in zip(jobs, paths)}
    report = {"rev_a": a.rev_a, "rev_b": a.rev_b, "units": {}}
    same = True
    for u in flags:
        ka, kb = hashes[(a.rev_a, u)], hashes[(a.rev_b, u)]
        rows = {}
        for k in list(ka) + [k for k in kb if k not in ka]:
            ok = ka.get(k) == kb.get(k)
            same = same and ok
            rows[k] = {"identical": ok, "sha256_a": ka.get(k), "sha256_b": kb.get(k)}
            print(f"unit {u}  {'identical' if ok else 'DIFFERS  '}  {k}")
        report["units"][u] = {"flags": " ".join(flags[u]).replace(ROOT, "."), "kernels": rows}
    n = sum(len(v["kernels"]) - 1 for v in report["units"].values())
    report["identical"] = same
    print(f"{n} kernels in {len(flags)} units: " + ("every one identical" if same else "NOT identical"))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
