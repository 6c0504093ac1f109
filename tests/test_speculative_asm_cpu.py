"""CPU: the static assembly checks of tests/test_wstream_asm_cpu.py over the units speculative decoding adds -- the ROWS
instantiation of the pipelined decode attention (ze_attn_rows.hip: no instruction may touch a Q / K register whose load is in
flight, tools/check_attn_asm.py) and the MFMA hazard rules over it and over ze_spec.hip (tools/check_mfma_hazards.py)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zoomearth_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-strict-aliasing", "-fno-slp-vectorize", "-I" + os.path.join(ROOT, "include"),
         "-I" + CSRC, "--cuda-device-only", "-S"]   # (the Makefile's)


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    d = tmp_path_factory.mktemp("specasm")
    out = {}
    for unit in ("ze_attn_rows", "ze_spec"):
        out[unit] = str(d / (unit + ".s"))
        r = subprocess.run([HIPCC] + FLAGS + [os.path.join(CSRC, unit + ".hip"), "-o", out[unit]], capture_output=True, text=True, timeout=1500)
        assert r.returncode == 0, (unit, r.stderr[-2000:])
    return out


def _run(tool, *paths):
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool)] + list(paths), capture_output=True, text=True)


def test_the_rows_attention_touches_no_load_in_flight(asm):
    c = _run("check_attn_asm.py", asm["ze_attn_rows"])
    assert c.returncode == 0, c.stdout[-3000:]
    lines = [ln for ln in c.stdout.splitlines() if "vector-memory operations" in ln]
    assert len(lines) == 1 and "wave_long" in lines[0] and " 0 early touches" in lines[0], c.stdout[-2000:]


def test_no_mfma_hazard_in_the_new_units(asm):
    c = _run("check_mfma_hazards.py", *asm.values())
    assert c.returncode == 0, c.stdout[-4000:]
    tot = [ln for ln in c.stdout.splitlines() if ln.endswith(" hazards")]
    assert len(tot) == 2 and all(ln.endswith(" 0 hazards") for ln in tot), c.stdout[-2000:]
