"""The lane record builder (csrc/zb_host.cpp build_lane_record) under AddressSanitizer and
UndefinedBehaviorSanitizer, on the CPU: `make constrec_selftest` builds the stand-alone driver
csrc/zb_constrec_selftest.cpp, which builds the record of the default and of the limbs model and
checks every word against the ZbModel row it has to come from, and the layout's alignment and
padding. No GPU and nothing loaded into Python: the driver is a program of its own.
"""

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ksim-gym-zbot_amd", "csrc")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def test_lane_record_builder_under_sanitizers(tmp_path, cmodel):
    from zbot_amd import compile_model
    from zbot_amd.mjcf import load_mjcf

    subprocess.run(["make", "-C", CSRC, "-s", "constrec_selftest"], check=True)
    limbs = compile_model(load_mjcf(os.path.join(ROOT, "ksim-gym-zbot_amd", "assets", "zbot_like_limbs.xml")))
    paths = []
    for name, cm in (("default", cmodel), ("limbs", limbs)):
        p = tmp_path / f"{name}.bin"
        p.write_bytes(bytes(cm.cmodel))
        paths.append(str(p))
    r = subprocess.run([os.path.join(CSRC, "build", "zb_constrec_selftest"), *paths], capture_output=True, text=True,
                       timeout=120, env=ENV)
    assert r.returncode == 0, f"rc={r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert "zb_constrec_selftest ok: 2 models" in r.stdout
    assert r.stdout.count(", 0 mismatches") == 2
