"""Test-side TIFF writer for the device decoder's tests: Pillow cannot be made to write tiles or chosen code streams.

A plain LZW encoder (TIFF 6.0: MSB-first, ClearCode 256, EOI 257, width one code early -- the rule of libtiff's encoder), a PackBits
encoder, the horizontal predictor and a minimal little-endian IFD, in strips or tiles.  Every file write_tiff() makes is opened with
Pillow and compared with its source array before it is handed out (check=True): that is what makes the writer trustworthy, and
tests/test_tiff_cpu.py runs it over every case the GPU tests use.  Also here: the image contents and the list of cases both test
files share, and the chunk files the sanitizer program (tests/tiff_san) reads.
"""
import os
import struct
import subprocess

import numpy as np

LZW, PACKBITS, DEFLATE = 5, 32773, 8
W, H = 67, 41   # widths divide nothing


# ---------------------------------------------------------------------------------------------------------------- encoders
class _Bits:
    def __init__(self):
        self.out, self.acc, self.n, self.codes = bytearray(), 0, 0, 0

    def put(self, code, width):
        self.acc = (self.acc << width) | code
        self.n += width
        self.codes += 1
        while self.n >= 8:
            self.n -= 8
            self.out.append((self.acc >> self.n) & 255)
        self.acc &= (1 << self.n) - 1

    def finish(self):
        if self.n:
            self.out.append((self.acc << (8 - self.n)) & 255)
        return bytes(self.out)


def lzw_encode(data: bytes, full_table_codes=None, clear_every=0, eoi=True):
    """(stream, number of codes) of TIFF LZW.  Default: a ClearCode when the next free code reaches 4094, as libtiff writes.
    full_table_codes = n: the table is allowed to fill (entries up to 4095) and n more codes go out at 12 bits before the ClearCode
    (a decoder has to go on with a full table and add nothing); -1: never a ClearCode after the table fills.  clear_every = n: a
    ClearCode after every n codes."""
    b = _Bits()
    b.put(256, 9)
    table, nxt, width, since_clear, at_full = {}, 258, 9, 0, 0

    def reset():
        nonlocal table, nxt, width, since_clear, at_full
        table, nxt, width, since_clear, at_full = {}, 258, 9, 0, 0

    def emitted():   # behind every code but Clear / EOI: the table entry, the width rule, the ClearCode policies
        nonlocal nxt, width, since_clear, at_full
        since_clear += 1
        clear = False
        if nxt < 4096:
            nxt += 1
            if full_table_codes is None and nxt == 4094:
                clear = True
            elif nxt > (1 << width) - 1 and width < 12:
                width += 1
        else:
            at_full += 1
            clear = full_table_codes is not None and full_table_codes >= 0 and at_full >= full_table_codes
        if clear_every and since_clear >= clear_every:
            clear = True
        if clear:
            b.put(256, width)
            reset()
        return clear

    if not data:
        if eoi:
            b.put(257, width)
        return b.finish(), b.codes
    omega = data[0]
    for k in data[1:]:
        key = (omega, k)
        if key in table:
            omega = table[key]
            continue
        b.put(omega, width)
        if nxt < 4096:
            table[key] = nxt
        emitted()
        omega = k
    b.put(omega, width)
    emitted()
    if eoi:
        b.put(257, width)
    return b.finish(), b.codes


def packbits_encode_row(row: bytes) -> bytes:
    out, i, n = bytearray(), 0, len(row)
    while i < n:
        j = i
        while j + 1 < n and row[j + 1] == row[i] and j - i < 127:
            j += 1
        if j > i:                          # a run of j - i + 1 in 2 .. 128
            out += bytes((257 - (j - i + 1), row[i]))
            i = j + 1
            continue
        j = i                              # literals until a run of three starts (or 128 of them)
        while j < n and j - i < 128 and not (j + 2 < n and row[j] == row[j + 1] == row[j + 2]):
            j += 1
        out += bytes((j - i - 1,)) + row[i:j]
        i = j
    return bytes(out)


def predict2(block: np.ndarray) -> np.ndarray:
    """The horizontal differencing of predictor 2 on a stored [rows, cols, 3] u8 block (rows restart at every chunk row)."""
    out = block.copy()
    out[:, 1:] = block[:, 1:] - block[:, :-1]   # uint8 arithmetic wraps mod 256
    return out


def compress_block(block: np.ndarray, compression: int, predictor: int = 1, **lzw_opts):
    """(bytes, codes) of one stored block [rows, cols, 3]."""
    if predictor == 2:
        block = predict2(block)
    if compression == LZW:
        return lzw_encode(block.tobytes(), **lzw_opts)
    assert compression == PACKBITS and not lzw_opts
    return b"".join(packbits_encode_row(r.tobytes()) for r in block), 0


# ---------------------------------------------------------------------------------------------------------------- the file
def _ifd(entries, data_start):
    """entries: {tag: (type, values)}; returns (ifd bytes placed at data_start, extra data behind it)."""
    sizes = {3: 2, 4: 4}
    fmt = {3: "H", 4: "I"}
    n = len(entries)
    extra_at = data_start + 2 + 12 * n + 4
    body, extra = struct.pack("<H", n), b""
    for tag in sorted(entries):
        typ, vals = entries[tag]
        raw = struct.pack("<%d%s" % (len(vals), fmt[typ]), *vals)
        if len(raw) <= 4:
            field = raw.ljust(4, b"\0")
        else:
            field = struct.pack("<I", extra_at + len(extra))
            extra += raw + (b"\0" if len(raw) % 2 else b"")
        body += struct.pack("<HHI", tag, typ, len(vals)) + field
    return body + struct.pack("<I", 0), extra


def write_tiff(path, arr, compression=LZW, predictor=1, layout=("strips", 4), check=True, chunks_override=None, extra_tags=None, **lzw_opts):
    """Writes arr u8 [h, w, 3] as an RGB TIFF.  layout: ("strips", rows per strip) or ("tiles", tile w, tile h) -- edge tiles padded with
    zeros to the tile size.  Returns the code count of every LZW chunk.  chunks_override {index: bytes} replaces chunks (defective
    files); check: the file must open under Pillow and equal arr."""
    arr = np.ascontiguousarray(arr, dtype=np.uint8)
    h, w = arr.shape[:2]
    blocks = []
    if layout[0] == "strips":
        rps = min(int(layout[1]), h)
        blocks = [arr[y:y + rps] for y in range(0, h, rps)]
    else:
        tw, th = int(layout[1]), int(layout[2])
        for y in range(0, h, th):
            for x in range(0, w, tw):
                t = np.zeros((th, tw, 3), dtype=np.uint8)
                part = arr[y:y + th, x:x + tw]
                t[:part.shape[0], :part.shape[1]] = part
                blocks.append(t)
    done = [compress_block(b, compression, predictor, **lzw_opts) for b in blocks]
    chunks = [d[0] for d in done]
    for i, raw in (chunks_override or {}).items():
        chunks[i] = raw
    entries = {256: (4, [w]), 257: (4, [h]), 258: (3, [8, 8, 8]), 259: (3, [compression]), 262: (3, [2]), 277: (3, [3]), 284: (3, [1])}
    if predictor != 1:
        entries[317] = (3, [predictor])
    entries.update(extra_tags or {})
    off_tag, cnt_tag = (273, 279) if layout[0] == "strips" else (324, 325)
    if layout[0] == "strips":
        entries[278] = (4, [rps])
    else:
        entries[322], entries[323] = (4, [tw]), (4, [th])
    entries[off_tag] = (4, [0] * len(chunks))
    entries[cnt_tag] = (4, [len(c) for c in chunks])
    ifd, extra = _ifd(entries, 8)
    at = 8 + len(ifd) + len(extra)
    offs = []
    for c in chunks:
        offs.append(at)
        at += len(c) + (len(c) & 1)
    entries[off_tag] = (4, offs)
    ifd, extra = _ifd(entries, 8)
    with open(path, "wb") as f:
        f.write(b"II*\0" + struct.pack("<I", 8) + ifd + extra)
        for c in chunks:
            f.write(c + (b"\0" if len(c) & 1 else b""))
    if check:
        assert np.array_equal(pillow_rgb(path), arr), f"{path}: Pillow does not read back what the writer was given"
    return [d[1] for d in done]


def pillow_rgb(path) -> np.ndarray:
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB")).copy()


def pillow_write(path, arr, compression, predictor=1, rows_per_strip=None):
    """The same through Pillow + libtiff (strips only): compression "tiff_lzw" / "packbits" / "tiff_adobe_deflate" / "raw"."""
    from PIL import Image, TiffImagePlugin
    old = TiffImagePlugin.STRIP_SIZE
    try:
        if rows_per_strip:
            TiffImagePlugin.STRIP_SIZE = rows_per_strip * (arr.size // arr.shape[0]) * arr.itemsize
        kw = {"tiffinfo": {317: 2}} if predictor == 2 else {}
        Image.fromarray(arr).save(path, format="TIFF", compression=compression, **kw)
    finally:
        TiffImagePlugin.STRIP_SIZE = old


# ---------------------------------------------------------------------------------------------------------------- contents and cases
def content(kind: str, h=H, w=W) -> np.ndarray:
    rng = np.random.default_rng(20240 + sum(map(ord, kind)))
    if kind == "colour":      # one colour: strings grow past 64 bytes at distance 3
        return np.broadcast_to(np.array([200, 17, 96], dtype=np.uint8), (h, w, 3)).copy()
    if kind == "greyrows":    # R = G = B, constant along a row: distance 1
        return np.broadcast_to(rng.integers(0, 256, (h, 1, 1), dtype=np.uint8), (h, w, 3)).copy()
    if kind in ("noise", "noise_full"):
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "gradient":    # smooth: small differences under predictor 2
        y, x = np.mgrid[0:h, 0:w]
        return np.stack([(2 * x + y) % 256, (x + 3 * y) % 256, (255 - x - y) % 256], axis=2).astype(np.uint8)
    raise KeyError(kind)


LAYOUTS = {"rps1": ("strips", 1), "rps4": ("strips", 4), "one": ("strips", H), "t16": ("tiles", 16, 16), "t32x16": ("tiles", 32, 16)}
SCHEMES = {"lzw": (LZW, 1), "lzw2": (LZW, 2), "packbits": (PACKBITS, 1)}


def cases():
    """[(id, content, layout name, scheme name, writer)]: each content x each layout x {LZW, LZW + predictor 2, PackBits} where the
    combination exists -- the gradient is the predictor-2 content, the no-ClearCode stream is LZW's -- written by the test writer, and
    the strip layouts once more by Pillow's own encoder."""
    out = []
    for c in ("colour", "greyrows", "noise"):
        for lay in LAYOUTS:
            for sch in SCHEMES:
                out.append((f"{c}-{lay}-{sch}", c, lay, sch, "ref"))
    for lay in LAYOUTS:
        out.append((f"gradient-{lay}-lzw2", "gradient", lay, "lzw2", "ref"))
        out.append((f"noise_full-{lay}-lzw", "noise_full", lay, "lzw", "ref"))
    for c, sch in (("noise", "lzw"), ("gradient", "lzw2"), ("greyrows", "packbits"), ("colour", "lzw2")):
        for lay in ("rps1", "rps4", "one"):
            out.append((f"{c}-{lay}-{sch}-pillow", c, lay, sch, "pillow"))
    return out


# a full table is carried for this many codes before the ClearCode of the "noise_full" content: libtiff's decoder keeps a table of
# 4096 + 1023 entries and stops at its end, so a file that Pillow must still read cannot go on for ever
FULL_TABLE_CODES = 900


def make_case(dirname, case):
    """Writes the case's file; returns (path, source array, code counts)."""
    cid, c, lay, sch, writer = case
    arr = content(c)
    path = os.path.join(dirname, cid + ".tif")
    comp, pred = SCHEMES[sch]
    if writer == "pillow":
        pillow_write(path, arr, {"lzw": "tiff_lzw", "lzw2": "tiff_lzw", "packbits": "packbits"}[sch], pred, LAYOUTS[lay][1])
        assert np.array_equal(pillow_rgb(path), arr)
        return path, arr, []
    opts = {"full_table_codes": FULL_TABLE_CODES} if c == "noise_full" else {}
    return path, arr, write_tiff(path, arr, comp, pred, LAYOUTS[lay], **opts)


# ---------------------------------------------------------------------------------------------------------------- the sanitizer program
SAN_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tiff_san", "ze_tiff_san.cpp")
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zoomearth_amd", "csrc")


def build_san(outdir):
    """The stand-alone CPU program over csrc/ze_tiff_codec.h, with AddressSanitizer and UBSan.  The sanitizer runtimes are linked
    statically, so the program runs directly whatever else the loader brings into the process and needs nothing preloaded.  g++ first, then
    clang++ (on the PATH, or the one the HIP toolchain that builds the library ships); no compiler that can build it is a failure, not a
    skip: these runs are the evidence for the decoder's bounds."""
    import shutil
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    tried = []
    for cxx, static in ((shutil.which("g++"), ["-static-libasan", "-static-libubsan"]), (shutil.which("clang++"), ["-static-libsan"]),
                        (os.path.join(rocm, "llvm", "bin", "clang++"), ["-static-libsan"])):
        if not cxx or not os.path.exists(cxx):
            continue
        exe = os.path.join(str(outdir), "ze_tiff_san")
        r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                            *static, "-I", CSRC, SAN_SRC, "-o", exe], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        tried.append((cxx, r.stderr[-1500:]))
    raise AssertionError(f"no host C++ compiler built the sanitizer program: {tried}")


def run_san(exe, chunks, workdir, name="cases"):
    """chunks: [(compression, compressed bytes, output bytes expected)] -> [(status, decoded bytes)] from ONE run of the program (which
    checks its own guard bytes on both sides of every output and exits non-zero when one changed)."""
    src, dst = os.path.join(str(workdir), name + ".in"), os.path.join(str(workdir), name + ".out")
    with open(src, "wb") as f:
        f.write(struct.pack("<I", len(chunks)))
        for comp, raw, n_out in chunks:
            f.write(struct.pack("<III", comp, len(raw), n_out) + raw)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "tiff codec ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    out = []
    with open(dst, "rb") as f:
        for comp, raw, n_out in chunks:
            (status,) = struct.unpack("<i", f.read(4))
            out.append((status, f.read(n_out)))
    return out


def plan_chunks(plan):
    """[(compression, bytes, stored bytes)] of a TiffPlan's chunks, read from its file."""
    buf = np.zeros(plan.n_bytes, dtype=np.uint8)
    assert plan.read_into(buf)
    return [(plan.compression, buf[o:o + n].tobytes(), int(sw) * int(sh) * 3) for o, n, _, _, _, _, sw, sh in plan.table.tolist()], buf


def assemble(plan, decoded):
    """The image from the decoded stored blocks of every chunk (predictor undone, tiles clipped): what the device's last kernel does."""
    img = np.zeros((plan.height, plan.width, 3), dtype=np.uint8)
    for (o, n, x0, y0, cw, ch, sw, sh), raw in zip(plan.table.tolist(), decoded):
        block = np.frombuffer(raw, dtype=np.uint8).reshape(sh, sw, 3)
        if plan.predictor == 2:
            block = np.cumsum(block, axis=1, dtype=np.uint8)
        img[y0:y0 + ch, x0:x0 + cw] = block[:ch, :cw]
    return img


# ---------------------------------------------------------------------------------------------------------------- reference decoders
# Independent of the codec header: strings are byte strings in a Python list, not offsets into the output.  Same status words.
OK, IN_EXHAUSTED, BAD_CODE, OUT_OVERRUN, OUT_SHORT, BAD_TABLE = 0, 1, 2, 3, 4, 5


def lzw_decode_ref(data: bytes, out_len: int):
    """(status, bytes decoded before the end) of a TIFF LZW stream that has to fill out_len bytes."""
    out, table, width, acc, nbits, pos, prev = bytearray(), None, 9, 0, 0, 0, None

    def fresh():
        return [bytes((i,)) for i in range(256)] + [b"", b""]

    table = fresh()
    while True:
        if len(out) == out_len:
            return OK, bytes(out)
        while nbits < width:
            if pos >= len(data):
                return IN_EXHAUSTED, bytes(out)
            acc, nbits, pos = (acc << 8) | data[pos], nbits + 8, pos + 1
        nbits -= width
        code = (acc >> nbits) & ((1 << width) - 1)
        acc &= (1 << nbits) - 1
        if code == 257:
            return OUT_SHORT, bytes(out)
        if code == 256:
            table, width, prev = fresh(), 9, None
            continue
        if code < 256:
            s = table[code]
        elif prev is None or code > len(table):
            return BAD_CODE, bytes(out)
        elif code < len(table):
            s = table[code]
        else:
            s = prev + prev[:1]
        if len(out) + len(s) > out_len:
            return OUT_OVERRUN, bytes(out)
        if prev is not None and len(table) < 4096:
            table.append(prev + s[:1])
            if len(table) >= (1 << width) - 1 and width < 12:
                width += 1
        out += s
        prev = s


def packbits_decode_ref(data: bytes, out_len: int):
    out, pos = bytearray(), 0
    while True:
        if len(out) == out_len:
            return OK, bytes(out)
        if pos >= len(data):
            return IN_EXHAUSTED, bytes(out)
        n, pos = data[pos], pos + 1
        if n == 128:
            continue
        if n < 128:
            if n + 1 > len(data) - pos:
                return IN_EXHAUSTED, bytes(out)
            if n + 1 > out_len - len(out):
                return OUT_OVERRUN, bytes(out)
            out += data[pos:pos + n + 1]
            pos += n + 1
        else:
            if pos >= len(data):
                return IN_EXHAUSTED, bytes(out)
            if 257 - n > out_len - len(out):
                return OUT_OVERRUN, bytes(out)
            out += bytes((data[pos],)) * (257 - n)
            pos += 1


def pack_codes(codes, width=9):
    """A stream of fixed-width codes (hand-made defective streams)."""
    b = _Bits()
    for c in codes:
        b.put(c, width)
    return b.finish()


def prefetcher_corrupt_chunk():
    """(image, index of the strip, its defective bytes, its stored size): the gradient in 4-row strips under predictor 2, strip 3 cut short by
    an EOI after 300 bytes.  The GPU test of the prefetcher's fall-back writes this file; defective_streams() puts the same bytes through the
    sanitizer program, which has to report "output short"."""
    arr = content("gradient")
    strip = predict2(arr[12:16]).tobytes()
    return arr, 3, lzw_encode(strip[:300])[0], len(strip)


def defective_streams():
    """[(name, compression, bytes, output bytes, status the issue names or None = whatever the reference decoder says)], fixed seeds."""
    rng = np.random.default_rng(77)
    out = []
    row = rng.integers(0, 256, 201, dtype=np.uint8).tobytes()                # a short chunk: one 67-px row of noise
    good, _ = lzw_encode(row)
    for cut in range(len(good)):                                             # truncation at every byte
        out.append((f"lzw-cut{cut}", LZW, good[:cut], 201, None))
    smooth = bytes((i // 7) & 255 for i in range(600))
    good2, _ = lzw_encode(smooth)
    for bit in rng.choice(len(good2) * 8, 160, replace=False).tolist():      # single flipped bits
        bad = bytearray(good2)
        bad[bit >> 3] ^= 0x80 >> (bit & 7)
        out.append((f"lzw-flip{bit}", LZW, bytes(bad), 600, None))
    out.append(("lzw-code-above-next", LZW, pack_codes([256, 65, 300]), 64, BAD_CODE))
    out.append(("lzw-code-just-above-next", LZW, pack_codes([256, 65, 66, 260]), 64, BAD_CODE))
    out.append(("lzw-table-code-first", LZW, pack_codes([256, 258]), 64, BAD_CODE))
    out.append(("lzw-longer-than-rectangle", LZW, lzw_encode(bytes(300))[0], 250, OUT_OVERRUN))
    _, _, early, n_strip = prefetcher_corrupt_chunk()
    out.append(("lzw-prefetcher-corrupt-chunk", LZW, early, n_strip, OUT_SHORT))
    out.append(("lzw-eoi-too-early", LZW, lzw_encode(row[:100])[0], 200, OUT_SHORT))
    out.append(("lzw-no-eoi-no-data", LZW, lzw_encode(row[:100], eoi=False)[0], 200, IN_EXHAUSTED))
    out.append(("lzw-only-clears", LZW, pack_codes([256] * 40), 16, IN_EXHAUSTED))
    pb = b"".join(packbits_encode_row(bytes(r)) for r in (row[:67], bytes(67), row[67:134]))
    for cut in range(len(pb)):
        out.append((f"packbits-cut{cut}", PACKBITS, pb[:cut], 201, None))
    for bit in rng.choice(len(pb) * 8, 120, replace=False).tolist():
        bad = bytearray(pb)
        bad[bit >> 3] ^= 0x80 >> (bit & 7)
        out.append((f"packbits-flip{bit}", PACKBITS, bytes(bad), 201, None))
    out.append(("packbits-run-crosses-end", PACKBITS, bytes((0x81, 7)), 100, OUT_OVERRUN))
    out.append(("packbits-literal-crosses-end", PACKBITS, bytes((9,)) + bytes(10), 8, OUT_OVERRUN))
    out.append(("packbits-literal-past-input", PACKBITS, bytes((5, 1, 2)), 8, IN_EXHAUSTED))
    out.append(("packbits-run-without-byte", PACKBITS, bytes((0xF0,)), 32, IN_EXHAUSTED))
    out.append(("packbits-only-noops", PACKBITS, bytes((128,)) * 50, 4, IN_EXHAUSTED))
    return out
