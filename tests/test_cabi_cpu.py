"""CPU: the C-ABI library loads, exports every symbol include/zoomearth.h declares, and its host-only
integer helpers (no GPU involved) reproduce the transformers golden vectors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

from zoomearth_amd import _lib
from zoomearth_amd.config import ModelConfig
from zoomearth_amd.engine import Engine


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_exports_match_header(lib):
    hdr = open(os.path.join(ROOT, "include", "zoomearth.h")).read()
    declared = set(re.findall(r"^(?:int|const char\*)\s+(ze_[a-z_0-9]+)\s*\(", hdr, flags=re.M))
    assert len(declared) >= 28
    assert declared == set(_lib.EXPORTS)
    for name in declared:
        assert getattr(lib, name) is not None
    assert lib.ze_version() >= 100


def _zcfg():
    return Engine._make_zcfg(ModelConfig.tiny(), 2, 256, 1024, 1024)


def test_smart_resize_host(lib, golden_json):
    for row in golden_json("indices.json")["smart_resize"]:
        oh, ow = C.c_int(), C.c_int()
        assert lib.ze_smart_resize(row["h"], row["w"], 28, 3136, row["max_pixels"], C.byref(oh), C.byref(ow)) == 0
        assert [oh.value, ow.value] == row["out"], row
    assert lib.ze_smart_resize(10, 5000, 28, 3136, 12845056, C.byref(oh), C.byref(ow)) < 0
    assert b"aspect ratio" in lib.ze_last_error(None)


def test_window_index_host(lib, golden_json):
    z = _zcfg()
    for row in golden_json("indices.json")["vision"]:
        g = np.asarray(row["grid"], dtype=np.int32)
        n = int((g[:, 0] * g[:, 1] * g[:, 2]).sum()) // 4
        wi = np.zeros(n, dtype=np.int64)
        cu = np.zeros(n + 2, dtype=np.int32)
        ncu = C.c_int()
        rc = lib.ze_vision_window_index(C.byref(z), g.ctypes.data_as(C.POINTER(C.c_int32)), len(g),
                                        wi.ctypes.data_as(C.POINTER(C.c_int64)),
                                        cu.ctypes.data_as(C.POINTER(C.c_int32)), len(cu), C.byref(ncu))
        assert rc == 0
        assert wi.tolist() == row["window_index"]
        assert cu[: ncu.value].tolist() == row["cu_window_seqlens"]


def test_rope_index_host(lib, golden_json):
    z = _zcfg()
    seen = 0
    for row in golden_json("indices.json")["rope_index"]:
        ids = np.asarray(row["input_ids"])
        am = np.asarray(row["attention_mask"])
        grids = np.asarray(row["grids"], dtype=np.int32)
        gi = 0
        for b in range(ids.shape[0]):
            cur = ids[b][am[b].astype(bool)].astype(np.int32)
            n_img = int(((cur == z.image_token_id) & (np.roll(cur, 1) != z.image_token_id)).sum())
            g = np.ascontiguousarray(grids[gi: gi + n_img])
            gi += n_img
            pos = np.zeros((3, len(cur)), dtype=np.int32)
            d = C.c_int32()
            rc = lib.ze_rope_index(C.byref(z), cur.ctypes.data_as(C.POINTER(C.c_int32)), len(cur),
                                   g.ctypes.data_as(C.POINTER(C.c_int32)), n_img,
                                   pos.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(d))
            assert rc == 0
            want = np.asarray(row["position_ids"])[:, b][:, am[b].astype(bool)]
            assert pos.tolist() == want.tolist()
            assert d.value == row["rope_deltas"][b][0]
            seen += 1
    assert seen >= 6
    bad = np.array([5, z.image_token_id, z.image_token_id, 7], dtype=np.int32)
    g = np.array([[1, 4, 4]], dtype=np.int32)
    pos = np.zeros((3, 4), dtype=np.int32)
    d = C.c_int32()
    assert lib.ze_rope_index(C.byref(z), bad.ctypes.data_as(C.POINTER(C.c_int32)), 4, g.ctypes.data_as(C.POINTER(C.c_int32)),
                             1, pos.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(d)) == -5


def test_host_helpers_under_asan_ubsan(tmp_path):
    """SURVEY.md section 5 (sanitizers; VERDICT r3 missing #5): zoomearth_amd/csrc/ze_index.cpp -- every integer index builder and
    the bicubic tap tables of the host side -- compiled with gcc -fsanitize=address,undefined and run against the golden vectors
    in a child process (libasan preloaded under the interpreter).  Any report (heap overflow, signed overflow, bad shift,
    misaligned access ...) aborts the child.  GPU sanitizers are not available on the pool, so this is the CPU build only."""
    import shutil
    import subprocess
    import sys
    gxx = shutil.which("g++")
    asan = subprocess.run([gxx, "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip() if gxx else ""
    if not gxx or not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("no g++ / libasan in this image")
    so = str(tmp_path / "libze_index_san.so")
    csrc = os.path.join(ROOT, "zoomearth_amd", "csrc")
    r = subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-fno-omit-frame-pointer", "-I", csrc, os.path.join(csrc, "ze_index.cpp"),
                        os.path.join(ROOT, "tests", "cabi_san", "ze_index_san.cpp"), "-o", so], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, LD_PRELOAD=asan, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cabi_san", "run_san.py"), so], capture_output=True, text=True,
                       env=env, timeout=600)
    assert r.returncode == 0 and "sanitized host helpers ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_no_product_path_flips_a_process_wide_tuning_knob():
    """`ze_tune` has no engine argument -- it is process-wide and measurement-only (include/zoomearth.h says so) -- so
    nothing a user imports may call it: not the Engine, the scheduler, the model / lane code, the server or the entry points.  (bench.py,
    tools/ and tests/ are measurement code and do.)"""
    import glob
    import re
    files = glob.glob(os.path.join(ROOT, "zoomearth_amd", "*.py")) + glob.glob(os.path.join(ROOT, "src", "**", "*.py"), recursive=True)
    assert len(files) > 10
    offenders = []
    for f in files:
        with open(f, encoding="utf-8") as fh:
            src = fh.read()
        if os.path.basename(f) == "_lib.py":
            src = re.sub(r'"ze_tune":.*', "", src)   # (the binding table itself)
        if re.search(r"\bze_tune\s*\(", src):
            offenders.append(os.path.relpath(f, ROOT))
    assert not offenders, offenders


def test_the_committed_counter_profile_names_the_kernel_sources_it_was_taken_on():
    """profiles/traffic_latest.json carries the hash of the library sources the PMC passes ran on; bench.py compares it with
    the tree that quotes the figure (`roofline.traffic_source`).  The hash function is a pure function of the source files."""
    import json
    from zoomearth_amd import _lib
    a, b = _lib.kernel_sources_sha16(), _lib.kernel_sources_sha16()
    assert a == b and len(a) == 16 and int(a, 16) >= 0
    with open(os.path.join(ROOT, "profiles", "traffic_latest.json")) as f:
        tj = json.load(f)
    assert tj.get("round", 0) >= 6 and len(tj.get("kernel_sources_sha16", "")) == 16
    assert tj["stream_shared"]["attention"]["ratio"] < tj["stream"]["attention"]["ratio"]


def test_ze_tune_bounds_and_the_knob_table_of_the_header(lib):
    """ze_tune takes the knobs 0 .. 24 and refuses the numbers beside them; the table of include/zoomearth.h names every enumerator of
    csrc/ze_knobs.h exactly once, with the same number (both files read as text)."""
    for k in range(25):
        assert lib.ze_tune(k, 0) == 0, k
    for k in (-1, 25):
        assert lib.ze_tune(k, 0) == -1, k   # ZE_ERR_INVALID
        assert b"unknown knob" in lib.ze_last_error(None)
    knobs_h = open(os.path.join(ROOT, "zoomearth_amd", "csrc", "ze_knobs.h")).read()
    enum = dict((name, int(num)) for name, num in re.findall(r"^\s+(ZE_KNOB_[A-Z0-9_]+) = (\d+),?", knobs_h, flags=re.M))
    assert enum.pop("ZE_KNOB_COUNT") == 25 and sorted(enum.values()) == list(range(25))
    hdr = open(os.path.join(ROOT, "include", "zoomearth.h")).read()
    rows = re.findall(r"^ \*\s+(\d+)\s+(ZE_KNOB_[A-Z0-9_]+)\b", hdr, flags=re.M)
    assert sorted((name, int(num)) for num, name in rows) == sorted(enum.items())
    for name in enum:
        assert len(re.findall(r"\b%s\b" % name, hdr)) == 1, name
