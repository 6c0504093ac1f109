"""CPU: the host side of the device TIFF decoder -- the test writer against Pillow, tiff_plan against Pillow's tags, the codec header
(zoomearth_amd/csrc/ze_tiff_codec.h: the state machines the kernels run) under AddressSanitizer + UBSan in a stand-alone program, over the
GPU tests' files and over defective streams, and the two new exports."""
import ctypes as C
import os

import numpy as np
import pytest

import tiff_ref as T
from zoomearth_amd import _lib
from zoomearth_amd.image import TiffPlan, decode_rgb, tiff_plan


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("tiff"))
    return {case[0]: (case,) + T.make_case(d, case) for case in T.cases()}   # make_case checks every file against Pillow


@pytest.fixture(scope="module")
def san(tmp_path_factory):
    d = tmp_path_factory.mktemp("tiff_san")
    return T.build_san(d), d   # (fails when no compiler can build it)


def test_every_file_of_the_writer_decodes_under_pillow(files):
    assert len(files) == len(T.cases()) >= 60
    # (c): one strip of uniform noise runs through all three width changes, fills the table and takes a ClearCode mid-chunk
    case, path, arr, codes = files["noise-one-lzw"]
    assert arr.nbytes == 8241 and len(codes) == 1 and codes[0] > 3838
    case, path, arr, codes = files["noise_full-one-lzw"]
    assert codes[0] > 3838 + T.FULL_TABLE_CODES   # the table filled and T.FULL_TABLE_CODES codes went out at 12 bits with nothing added
    assert {c[2] for c in T.cases()} == set(T.LAYOUTS) and {c[3] for c in T.cases()} == set(T.SCHEMES)


def test_tiff_plan_against_pillows_tags(files):
    from PIL import Image
    for cid, (case, path, arr, codes) in files.items():
        plan = tiff_plan(path)
        assert isinstance(plan, TiffPlan), cid
        with Image.open(path) as im:
            tags = dict(im.tag_v2)
        comp, pred = T.SCHEMES[case[3]]
        assert (plan.width, plan.height, plan.compression, plan.predictor) == (T.W, T.H, comp, pred), cid
        assert tags[259] == comp and tags.get(317, 1) == pred
        lay = T.LAYOUTS[case[2]]
        tab = plan.table
        if lay[0] == "tiles":
            tw, th = lay[1:]
            assert plan.tiled and (plan.chunk_w, plan.chunk_h) == (tw, th) == (tags[322], tags[323])
            assert plan.file_offsets.tolist() == list(tags[324]) and tab[:, 1].tolist() == list(tags[325])
            across, down = -(-T.W // tw), -(-T.H // th)
            assert plan.n_chunks == across * down
            for i, (o, n, x0, y0, cw, ch, sw, sh) in enumerate(tab.tolist()):
                assert (x0, y0) == ((i % across) * tw, (i // across) * th) and (sw, sh) == (tw, th)
                assert (cw, ch) == (min(tw, T.W - x0), min(th, T.H - y0))   # edge tiles: stored padded, placed clipped
        else:
            rps = tags[278]
            assert not plan.tiled and plan.chunk_w == T.W and plan.chunk_h == min(rps, T.H)
            assert plan.file_offsets.tolist() == list(tags[273]) and tab[:, 1].tolist() == list(tags[279])
            assert plan.n_chunks == -(-T.H // rps)
            for i, (o, n, x0, y0, cw, ch, sw, sh) in enumerate(tab.tolist()):
                assert (x0, y0, cw, sw) == (0, i * rps, T.W, T.W) and ch == sh == min(rps, T.H - y0)
        # the upload buffer: every chunk on a 16-byte boundary, none overlapping, the whole a multiple of 16
        assert (tab[:, 0] % 16 == 0).all() and plan.n_bytes % 16 == 0
        ends = tab[:, 0] + tab[:, 1]
        assert (ends[:-1] <= tab[1:, 0]).all() and ends[-1] <= plan.n_bytes


def test_tiff_plan_is_none_for_every_file_the_device_does_not_decode(tmp_path):
    from PIL import Image
    rgb = T.content("gradient")
    p = lambda n: str(tmp_path / n)
    T.pillow_write(p("deflate.tif"), rgb, "tiff_adobe_deflate")
    T.pillow_write(p("raw.tif"), rgb, "raw")
    T.pillow_write(p("rgba.tif"), np.dstack([rgb, rgb[:, :, :1]]), "tiff_lzw")
    T.pillow_write(p("grey.tif"), rgb[:, :, 0].copy(), "tiff_lzw")
    T.pillow_write(p("u16.tif"), rgb[:, :, 0].astype(np.uint16) * 257, "tiff_lzw")
    Image.fromarray(rgb).convert("P").save(p("palette.tif"), compression="tiff_lzw")
    Image.fromarray(rgb).save(p("jpeg.tif"), compression="jpeg")
    Image.fromarray(rgb).save(p("tile.png"))
    T.write_tiff(p("planar2.tif"), rgb, T.LZW, check=False, extra_tags={284: (3, [2])})
    T.write_tiff(p("fillorder2.tif"), rgb, T.LZW, check=False, extra_tags={266: (3, [2])})
    T.write_tiff(p("orient.tif"), rgb, T.LZW, check=False, extra_tags={274: (3, [3])})
    T.write_tiff(p("unknown_tag.tif"), rgb, T.LZW, check=False, extra_tags={65000: (3, [1])})
    good = T.lzw_encode(rgb[:4].tobytes())[0]
    T.write_tiff(p("old_lzw.tif"), rgb, T.LZW, check=False, chunks_override={0: b"\x00\x01" + good[2:]})
    T.write_tiff(p("old_lzw_later.tif"), rgb, T.LZW, check=False, chunks_override={3: b"\x00\x01" + good[2:]})
    big = np.zeros((8, 50000, 3), dtype=np.uint8)   # one strip row is fine, eight rows in a strip pass the 1 MiB a chunk may store
    T.write_tiff(p("big_chunk.tif"), big, T.PACKBITS, layout=("strips", 8), check=False)
    for name in ("deflate.tif", "raw.tif", "rgba.tif", "grey.tif", "u16.tif", "palette.tif", "jpeg.tif", "tile.png", "planar2.tif", "fillorder2.tif",
                 "orient.tif", "unknown_tag.tif", "old_lzw.tif", "big_chunk.tif", "missing.tif"):
        assert tiff_plan(p(name)) is None, name
    # old-style LZW in a later chunk shows when the chunks are read
    plan = tiff_plan(p("old_lzw_later.tif"))
    assert plan is not None and plan.read_into(np.zeros(plan.n_bytes, dtype=np.uint8)) is False
    # harmless tags (a description, a resolution) do not turn a file away; uncompressed files keep decode_rgb's own fast path
    T.write_tiff(p("described.tif"), rgb, T.LZW, extra_tags={296: (3, [2]), 254: (4, [0])})
    assert tiff_plan(p("described.tif")) is not None
    assert np.array_equal(decode_rgb(p("raw.tif")), rgb)


def test_codec_under_sanitizers_decodes_the_gpu_tests_files(files, san):
    exe, d = san
    chunks, owners = [], []
    for cid, (case, path, arr, codes) in files.items():
        plan = tiff_plan(path)
        mine, _ = T.plan_chunks(plan)
        owners.append((cid, plan, arr, len(chunks), len(mine)))
        chunks += mine
    got = T.run_san(exe, chunks, d, "files")    # one run of the program for all of them
    for cid, plan, arr, at, n in owners:
        part = got[at:at + n]
        assert [st for st, _ in part] == [0] * n, cid
        assert np.array_equal(T.assemble(plan, [raw for _, raw in part]), arr), cid


def test_codec_under_sanitizers_goes_on_with_a_full_table_that_is_never_cleared(san):
    """What Pillow cannot check (libtiff's decoder ends its table 1023 entries behind the last code): no ClearCode at all once the table is
    full.  The source bytes are the reference."""
    exe, d = san
    data = T.content("noise", 160, 67).tobytes()
    stream, codes = T.lzw_encode(data, full_table_codes=-1)
    assert codes > 3838 + 5000
    assert T.lzw_decode_ref(stream, len(data)) == (0, data)
    (st, raw), = T.run_san(exe, [(T.LZW, stream, len(data))], d, "never_cleared")
    assert st == 0 and raw == data
    every, _ = T.lzw_encode(data[:3000], clear_every=7)     # and a ClearCode every few codes
    (st, raw), = T.run_san(exe, [(T.LZW, every, 3000)], d, "clear_every")
    assert st == 0 and raw == data[:3000]


def test_codec_under_sanitizers_on_defective_streams(san):
    """Clean exit (no sanitizer report, the program's own guard bytes on both sides of every output intact -- it exits non-zero otherwise),
    and the status the defect has: the one the case names, which is also what the independent reference decoder of tiff_ref gives."""
    exe, d = san
    cases = T.defective_streams()
    assert len(cases) > 500
    got = T.run_san(exe, [(comp, raw, n) for _, comp, raw, n, _ in cases], d, "defects")
    seen = set()
    for (name, comp, raw, n, want), (st, out) in zip(cases, got):
        ref_st, ref_out = (T.lzw_decode_ref if comp == T.LZW else T.packbits_decode_ref)(raw, n)
        assert want is None or ref_st == want, name
        assert st == ref_st, (name, st, ref_st)
        assert out[:len(ref_out)] == ref_out, name                     # what was decoded before the defect
        assert out[len(ref_out):] == b"\xa5" * (n - len(ref_out)), name   # and nothing behind it was touched
        seen.add(st)
    assert seen == {0, 1, 2, 3, 4}
    cut = {name: st for (name, *_), (st, _) in zip(cases, got) if name.startswith("lzw-cut")}
    assert cut["lzw-cut0"] == 1 and set(cut.values()) <= {0, 1} and list(cut.values()).count(1) >= len(cut) - 2


def test_new_exports_are_present_and_refuse_null_or_zero_arguments():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.lib()
    assert {"ze_tile_upload_tiff", "ze_op_tiff_decode"} <= set(_lib.EXPORTS)
    buf = (C.c_uint8 * 64)()
    tab = (C.c_int32 * 8)()
    p, t = C.cast(buf, C.c_void_p), C.cast(tab, C.c_void_p)
    for fn in (lib.ze_tile_upload_tiff, lib.ze_op_tiff_decode):
        assert fn(None, p, 64, t, 1, 4, 4, 5, 1, 0, 4, 4, p, t, None) == -1      # ZE_ERR_INVALID: no engine
        assert b"null argument" in lib.ze_last_error(None)
        assert fn(None, None, 0, None, 0, 0, 0, 0, 0, 0, 0, 0, None, None, None) == -1
