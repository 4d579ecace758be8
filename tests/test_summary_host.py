"""TensorBoard summaries, the parts that need no GPU: the record framing and the hand-encoded protobufs against known-answer bytes, the
reader's CRC checks, scalar and PNG round trips (decoded by a decoder written here from zlib), the writer's queue, the NumPy
restatements of include/vnet_hip_summary.h, the tag rule, the ledger of the header and its error codes before any launch, and the
SummaryInterval key."""
import colorsys
import ctypes
import os
import struct
import threading
import time
import zlib

import numpy as np
import pytest

from tests import guard
from vnet_tensorflow_amd import summary as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "vnet_hip_summary.h")

# float32 bit patterns of softmax values at which a fused multiply-add of 6 * H - 3 / - 2 / - 4 (one rounding instead of two) changes an
# output byte of the rainbow rule: found on the CPU by comparing summary.rainbow with fused_rainbow below over 8 * 10^7 seeded uniform
# draws.  A kernel compiled with contraction passes every other input of tests/test_hip_summary.py; these it fails.
FMA_PROBES = (981500416, 1007718592, 1015580832, 1019791584, 1023706240, 1023706256, 1027916992, 1027917008, 1030022384, 1033015952,
              1033015960, 1035121336, 1036174016, 1038279400, 1039332080, 1039332088, 1040286080, 1040286084, 1040812424, 1040812428,
              1041865112, 1041865116, 1042391456, 1042391460, 1042917800, 1042917804, 1043444144, 1043970492, 1044496832, 1044496836,
              1045549520, 1045549524, 1046075868, 1046602212, 1047128552, 1048181240, 1048181244)


def fused_rainbow(p):
    """summary.rainbow with dh - 3, dh - 2 and dh - 4 formed from the EXACT product 6 * H (float64 holds it) and rounded once: what a
    contracted kernel computes."""
    p = np.asarray(p, np.float32)
    one, two = np.float32(1), np.float32(2)
    h = ((one - p) * two) / np.float32(3)
    e = h.astype(np.float64) * 6.0
    d3, d2, d4 = ((e - k).astype(np.float32) for k in (3.0, 2.0, 4.0))
    rgb = np.stack([np.clip(np.abs(d3) - one, 0, one), np.clip(two - np.abs(d2), 0, one), np.clip(two - np.abs(d4), 0, one)], -1)
    return S._bytes_of(rgb * np.float32(255))


def decode_png(png):
    """A PNG decoder for 8-bit grey / RGB, non-interlaced, all five filter types: uint8 [H, W] or [H, W, 3]."""
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, head, ended = 8, b"", None, False
    while pos < len(png):
        n, kind = struct.unpack(">I4s", png[pos:pos + 8])
        body = png[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", png[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + body) & 0xffffffff, kind
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat += body
        elif kind == b"IEND":
            ended = True
        pos += 12 + n
    assert ended and head is not None
    w, h, depth, ctype, comp, filt, lace = head
    assert depth == 8 and ctype in (0, 2) and (comp, filt, lace) == (0, 0, 0)
    bpp = 1 if ctype == 0 else 3
    raw = zlib.decompress(idat)
    stride = w * bpp
    assert len(raw) == h * (stride + 1)
    out = np.zeros((h, stride), dtype=np.uint8)
    prev = np.zeros(stride, dtype=np.int64)
    for r in range(h):
        ft = raw[r * (stride + 1)]
        line = np.frombuffer(raw, np.uint8, stride, r * (stride + 1) + 1).astype(np.int64)
        cur = np.zeros(stride, dtype=np.int64)
        for i in range(stride):
            a = cur[i - bpp] if i >= bpp else 0
            b = prev[i]
            c = prev[i - bpp] if i >= bpp else 0
            if ft == 0:
                pred = 0
            elif ft == 1:
                pred = a
            elif ft == 2:
                pred = b
            elif ft == 3:
                pred = (a + b) // 2
            else:
                pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
            cur[i] = (line[i] + pred) & 255
        out[r] = cur
        prev = cur
    return out.reshape(h, w) if bpp == 1 else out.reshape(h, w, 3)


# ---- framing -------------------------------------------------------------------------------------------------------------------------
EVENT_HEX = "09000000000000f03f10032a0a0a080a0161150000003f"
RECORD_HEX = "1700000000000000e7cef81e09000000000000f03f10032a0a0a080a0161150000003fa4692d17"


def test_known_answer_event_and_record(tmp_path):
    """Event{wall_time 1.0, step 3, summary{value{tag "a", simple_value 0.5}}} by hand:
      09                      field 1 (wall_time), wire type 1 (64-bit)      key = 1 << 3 | 1
      00 00 00 00 00 00 f0 3f the double 1.0, little endian
      10 03                   field 2 (step), wire type 0 (varint)           key = 2 << 3 | 0; 3
      2a 0a                   field 5 (summary), wire type 2                 key = 5 << 3 | 2; 10 bytes follow
        0a 08                 Summary field 1 (value), wire type 2; 8 bytes follow
          0a 01 61            Value field 1 (tag), wire type 2; 1 byte; "a"
          15 00 00 00 3f      Value field 2 (simple_value), wire type 5 (32-bit) key = 2 << 3 | 5; the float 0.5
    23 bytes; the record: uint64 23, masked crc32c of those 8 bytes, the 23 bytes, their masked crc32c (tf_checkpoint.crc32c, pinned
    to RFC 3720's check value by tests/test_tf_checkpoint.py)."""
    data = S.encode_event(1.0, 3, [("a", 0.5)])
    assert data.hex() == EVENT_HEX and len(data) == 23
    rec = S.encode_record(data)
    assert rec.hex() == RECORD_HEX and len(rec) == 39
    path = tmp_path / "one"
    path.write_bytes(rec)
    assert list(S.read_events(str(path))) == [(1.0, 3, {"a": 0.5})]
    # one flipped bit anywhere -- the length, its CRC, the data, its CRC -- is refused
    for byte in (0, 3, 8, 11, 12, 20, 34, 35, 38):
        for bit in (0, 7):
            bad = bytearray(rec)
            bad[byte] ^= 1 << bit
            path.write_bytes(bytes(bad))
            with pytest.raises(ValueError):
                list(S.read_events(str(path)))
    path.write_bytes(rec[:-1])
    with pytest.raises(ValueError):
        list(S.read_events(str(path)))
    path.write_bytes(rec + rec[:5])
    with pytest.raises(ValueError):
        list(S.read_events(str(path)))


def test_bulk_crc_is_the_byte_loop():
    """summary.crc32c_bulk (segments advanced together in NumPy, then combined) against tf_checkpoint.crc32c, below, at and above the
    size where it leaves the byte loop, with and without a head in front of the segments."""
    from vnet_tensorflow_amd.tf_checkpoint import crc32c
    rng = np.random.default_rng(4)
    L = S._CRC_LANES
    assert S.crc32c_bulk(b"123456789") == 0xe3069283
    for n in (0, 1, 16 * L - 1, 16 * L, 16 * L + 1, 17 * L + 4097, 40 * L + 7):
        d = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert S.crc32c_bulk(d) == crc32c(d), n
    d = bytes(40 * L)
    assert S.crc32c_bulk(d) == crc32c(d) and S.crc32c_bulk(b"\xff" * (33 * L)) == crc32c(b"\xff" * (33 * L))
    # a record past the threshold, as the writer frames it
    data = S.encode_event(2.0, 9, [("img", (600, 600, 1, S.encode_png(rng.integers(0, 256, (600, 600), dtype=np.uint8), level=0)))])
    assert len(data) > 16 * L
    rec = S.encode_record(data)
    assert rec[-4:] == struct.pack("<I", S.mask_crc(crc32c(data)))


# ---- round trips ---------------------------------------------------------------------------------------------------------------------
def test_round_trip_scalars_and_images(tmp_path):
    rng = np.random.default_rng(0)
    images = {}
    for h, w in ((1, 1), (5, 7), (33, 17)):
        images["grey_%dx%d" % (h, w)] = rng.integers(0, 256, (h, w), dtype=np.uint8)
        images["rgb_%dx%d" % (h, w)] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    scalars = [("loss/0.total_loss", np.float32(0.1)), ("metrics/accuracy", 1.0), ("learning_rate_1", np.float32(1e-3)),
               ("nan", float("nan")), ("big", np.float32(3.0e38))]
    w = S.FileWriter(str(tmp_path / "run"))
    steps = [1, 2, 7, 2 ** 40]
    for k, step in enumerate(steps):
        values = scalars[k:] + scalars[:k] + list(images.items())
        w.add_summary(values, step)
    w.flush()
    assert os.path.getsize(w.path) > 0
    w.close()
    w.close()                                                           # idempotent
    name = os.path.basename(w.path).split(".")
    assert name[:3] == ["events", "out", "tfevents"] and len(name[3]) == 10 and name[3].isdigit() and S.event_files(str(tmp_path)) == [w.path]
    assert S.file_version(w.path) == "brain.Event:2"
    events = list(S.read_events(w.path))
    first = S.parse_event(next(S.read_records(w.path)))
    assert first["file_version"] == "brain.Event:2" and first["values"] == [] and first["step"] == 0 and first["wall_time"] > 1e9
    assert events[0][1:] == (0, {}) and [e[1] for e in events[1:]] == steps
    try:
        from PIL import Image
    except ImportError:
        Image = None
    for k, (wall, step, values) in enumerate(events[1:]):
        assert abs(wall - time.time()) < 600
        assert list(values) == [t for t, _ in scalars[k:] + scalars[:k]] + list(images)             # tag order as written
        for tag, v in scalars:
            got = values[tag]
            assert isinstance(got, float) and (np.float32(got) == np.float32(v) or (got != got and v != v)), tag      # float32-exact
        for tag, pix in images.items():
            h, wd, cs, png = values[tag]
            assert (h, wd, cs) == (pix.shape[0], pix.shape[1], 1 if pix.ndim == 2 else 3)
            assert np.array_equal(decode_png(png), pix), tag
            if Image is not None:
                import io
                im = Image.open(io.BytesIO(png))
                assert im.mode == ("L" if pix.ndim == 2 else "RGB") and np.array_equal(np.asarray(im), pix), tag
    # the listing of python -m vnet_tensorflow_amd.summary
    rows = S.scalar_table(str(tmp_path))
    assert [(r[0], r[1]) for r in rows] == [("run", s) for s in steps] and set(rows[0][2]) == {t for t, _ in scalars}


def test_decoder_reads_every_filter_type():
    """The decoder above is not tied to the writer's filter type 0: a PNG assembled here with filters 1-4 decodes to the same pixels."""
    rng = np.random.default_rng(1)
    pix = rng.integers(0, 256, (6, 5, 3), dtype=np.uint8)
    h, w, bpp = 6, 5, 3
    raw = bytearray()
    flat = pix.reshape(h, -1).astype(np.int64)
    for r in range(h):
        ft = (0, 1, 2, 3, 4, 4)[r]
        raw.append(ft)
        for i in range(w * bpp):
            a = flat[r, i - bpp] if i >= bpp else 0
            b = flat[r - 1, i] if r else 0
            c = flat[r - 1, i - bpp] if r and i >= bpp else 0
            pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
            pred = (0, a, b, (a + b) // 2, a if pa <= pb and pa <= pc else (b if pb <= pc else c))[ft]
            raw.append(int(flat[r, i] - pred) & 255)
    png = b"\x89PNG\r\n\x1a\n" + S._chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + \
        S._chunk(b"IDAT", zlib.compress(bytes(raw))) + S._chunk(b"IEND", b"")
    assert np.array_equal(decode_png(png), pix) and np.array_equal(decode_png(S.encode_png(pix)), pix)
    with pytest.raises(ValueError):
        S.encode_png(pix.astype(np.int32))
    with pytest.raises(ValueError):
        S.encode_png(np.zeros((2, 2, 4), np.uint8))


# ---- the writer ----------------------------------------------------------------------------------------------------------------------
class _Gate(object):
    """Stands in for the event behind a device-to-host copy: synchronize() returns once the test opens the gate."""

    def __init__(self):
        self.open, self.waits = threading.Event(), 0

    def synchronize(self):
        self.waits += 1
        assert self.open.wait(60)


def test_full_queue_blocks_and_loses_nothing(tmp_path):
    N, Q = 25, 3
    w = S.FileWriter(str(tmp_path), max_queue=Q)
    gate = _Gate()
    done = []

    def produce():
        for k in range(N):
            w.add_summary([("k", float(k)), ("img", np.full((2, 3), k, np.uint8))], k + 1, wait=gate)
            done.append(k)
    t = threading.Thread(target=produce)
    t.start()
    deadline = time.time() + 60
    while len(done) < Q + 1 and time.time() < deadline:              # the worker holds one event at the gate, the queue Q more
        time.sleep(0.001)
    for _ in range(20):                                              # ... and the producer stays blocked on the next one
        time.sleep(0.001)
    assert len(done) == Q + 1 and t.is_alive()
    gate.open.set()
    t.join(60)
    assert not t.is_alive() and len(done) == N
    w.close()                                                          # drains
    events = list(S.read_events(w.path))[1:]
    assert [e[1] for e in events] == list(range(1, N + 1)) and [e[2]["k"] for e in events] == [float(k) for k in range(N)]
    assert all(np.array_equal(decode_png(e[2]["img"][3]), np.full((2, 3), k, np.uint8)) for k, e in enumerate(events))
    assert gate.waits == N
    with pytest.raises(ValueError):
        w.add_summary([("k", 0.0)], 1)


def test_close_drains_the_queue(tmp_path):
    w = S.FileWriter(str(tmp_path))
    gate = _Gate()
    for k in range(S.QUEUE_SIZE):
        w.add_summary([("k", float(k))], k + 1, wait=gate)
    threading.Timer(0.01, gate.open.set).start()
    w.close()
    assert [e[1] for e in S.read_events(w.path)][1:] == list(range(1, S.QUEUE_SIZE + 1))


def test_worker_exception_surfaces_on_the_caller(tmp_path):
    w = S.FileWriter(str(tmp_path))
    w.add_summary([("ok", 1.0)], 1)

    def boom():
        raise RuntimeError("encoder failed")
    w.add_summary([("bad", boom)], 2)
    with pytest.raises(RuntimeError, match="encoder failed"):
        w.flush()
    w.add_summary([("ok", 3.0)], 3)                                    # the writer goes on after the error was delivered
    w.add_summary([("bad", np.zeros((2, 2), np.float32))], 4)          # not uint8: encode_png refuses
    with pytest.raises(ValueError, match="encode_png"):
        for k in range(100):
            w.add_summary([("ok", 0.0)], 5 + k)
            time.sleep(0.001)
    with pytest.raises(RuntimeError, match="late"):
        w.add_summary([("bad", lambda: (_ for _ in ()).throw(RuntimeError("late")))], 200)
        w.close()
    w.close()
    steps = [e[1] for e in S.read_events(w.path)]
    assert steps[:2] == [0, 1] and 2 not in steps and 3 in steps and 4 not in steps and 200 not in steps


def test_restart_opens_a_new_file(tmp_path):
    a = S.FileWriter(str(tmp_path))
    b = S.FileWriter(str(tmp_path))
    a.close(), b.close()
    assert a.path != b.path and len(S.event_files(str(tmp_path))) == 2


def test_cli_lists_scalars(tmp_path, capsys):
    w = S.FileWriter(str(tmp_path / "train"))
    w.add_summary([("loss/0.total_loss", 0.25), ("img", np.zeros((2, 2), np.uint8))], 1)
    w.add_summary([("loss/0.total_loss", 0.125), ("learning_rate_1", 0.5)], 2)
    w.close()
    assert S.main([str(tmp_path)]) == 0
    out = capsys.readouterr().out.splitlines()
    assert out[0].split() == ["run", "step", "loss/0.total_loss", "learning_rate_1"]
    assert out[1].split() == ["train", "1", "0.25", "-"] and out[2].split() == ["train", "2", "0.125", "0.5"]
    assert S.main([]) == 2


# ---- the restatements ----------------------------------------------------------------------------------------------------------------
def test_rainbow_restatement():
    assert S.rainbow(np.float32([0.0, 0.5, 1.0])).tolist() == [[0, 0, 255], [0, 255, 0], [255, 0, 0]]
    grid = np.arange(1025, dtype=np.float32) / np.float32(1024)
    draws = np.random.default_rng(7).random(200000, dtype=np.float32)
    p = np.concatenate([grid, draws])
    got = S.rainbow(p).astype(np.int64)
    ref = np.empty_like(got)
    for i, v in enumerate(p.astype(np.float64)):
        ref[i] = [int(c * 255.0) for c in colorsys.hsv_to_rgb((1.0 - v) * 2.0 / 3.0, 1.0, 1.0)]
    assert np.abs(got - ref).max() <= 1
    assert S.rainbow(np.float32([np.nan])).tolist() == [[0, 0, 0]]
    sm = np.random.default_rng(8).random((2, 3, 4, 5, 2), dtype=np.float32)
    out = S.slices_rainbow(sm)
    assert out.shape == (2, 2, 5, 3, 4, 3) and out.dtype == np.uint8
    assert np.array_equal(out[1, 0, 4, 2, 3], S.rainbow(sm[1, 2, 3, 4, 0]))


def test_fma_probes_separate_the_two_roundings():
    p = np.array(FMA_PROBES, dtype=np.uint32).view(np.float32)
    assert len(set(FMA_PROBES)) >= 32 and ((p > 0) & (p < 1)).all()
    assert (S.rainbow(p) != fused_rainbow(p)).any(axis=-1).all()


def test_intensity_restatement():
    v = np.float32([-0.0, -1.0, 0.999, 255.0, 255.999, 256.0, 1e9, np.inf, -np.inf, np.nan, -0.5, 1.0, 17.9, 254.5, -1e9])
    assert S._bytes_of(v).tolist() == [0, 0, 0, 255, 255, 255, 255, 255, 0, 0, 0, 1, 17, 254, 0]
    x = np.random.default_rng(2).random((2, 3, 4, 5, 2), dtype=np.float32) * 300 - 20
    out = S.slices_intensity(x)
    assert out.shape == (2, 2, 5, 3, 4) and out.dtype == np.uint8
    for b, xx, y, z, c in ((0, 0, 0, 0, 0), (1, 2, 3, 4, 1), (0, 1, 2, 3, 1)):
        assert out[b, c, z, xx, y] == S._bytes_of(x[b, xx, y, z, c])


def test_index_restatement_and_factors():
    with_zero = {K: S.index_factor(K, list(range(K))) for K in range(2, 7)}
    without = {K: S.index_factor(K, list(range(1, K + 1))) for K in range(2, 7)}
    assert with_zero == {2: 255, 3: 127, 4: 85, 5: 63, 6: 51} and without == {2: 127, 3: 85, 4: 63, 5: 51, 6: 42}
    with pytest.raises(ValueError):
        S.index_factor(1, [0])
    for dtype in (np.int32, np.int64):
        lab = np.array([0, 1, 2, 3, 4, 5, 300, -1, np.iinfo(dtype).max, np.iinfo(dtype).min], dtype=dtype).reshape(1, 1, 1, 10, 1)
        for f in (255, 63, 42):
            want = [(int(v) * f) % 256 for v in lab.reshape(-1)]
            assert S.slices_index(lab, f).reshape(-1).tolist() == want
    lab = np.random.default_rng(3).integers(0, 5, (2, 3, 4, 5, 1)).astype(np.int32)
    out = S.slices_index(lab, 63)
    assert out.shape == (2, 1, 5, 3, 4) and out[1, 0, 4, 2, 3] == lab[1, 2, 3, 4, 0] * 63


# ---- tags ----------------------------------------------------------------------------------------------------------------------------
def test_tag_rule():
    assert S.image_tags("image.nii.gz_batch0", 3) == ["image.nii.gz_batch0/image/%d" % i for i in range(3)]
    assert S.image_tags("label_batch1", 1) == ["label_batch1/image"] and S.clean_tag("/a b:c") == "a_b_c"
    tags = S.step_tags(["t1.nii", "t2.nii"], [0, 1, 4], 2, 2, "mixed_sorensen", True)
    assert tags == [
        "t1.nii_batch0/image/0", "t1.nii_batch0/image/1", "t2.nii_batch0/image/0", "t2.nii_batch0/image/1",
        "label_batch0/image/0", "label_batch0/image/1",
        "t1.nii_batch1/image/0", "t1.nii_batch1/image/1", "t2.nii_batch1/image/0", "t2.nii_batch1/image/1",
        "label_batch1/image/0", "label_batch1/image/1",
        "softmax_0_batch0/image/0", "softmax_0_batch0/image/1", "softmax_1_batch0/image/0", "softmax_1_batch0/image/1",
        "softmax_4_batch0/image/0", "softmax_4_batch0/image/1",
        "softmax_0_batch1/image/0", "softmax_0_batch1/image/1", "softmax_1_batch1/image/0", "softmax_1_batch1/image/1",
        "softmax_4_batch1/image/0", "softmax_4_batch1/image/1",
        "loss/1.dice", "loss/2.regularized_xent", "loss/0.total_loss",
        "pred_batch0/image/0", "pred_batch0/image/1", "pred_batch1/image/0", "pred_batch1/image/1",
        "metrics/accuracy",
        "metrics/sensitivity_1", "metrics/specificity_1", "metrics/dice_1", "metrics/auc_1",
        "metrics/sensitivity_4", "metrics/specificity_4", "metrics/dice_4", "metrics/auc_4",
        "learning_rate_1"]
    assert S.step_tags(["t1.nii"], [0, 1], 2, 16, "sorensen", False) == [
        "loss/0.total_loss", "metrics/accuracy", "metrics/sensitivity_1", "metrics/specificity_1", "metrics/dice_1", "metrics/auc_1",
        "learning_rate_1"]


# ---- the ledger of include/vnet_hip_summary.h ----------------------------------------------------------------------------------------
def test_summary_header_ledger():
    """include/vnet_hip_summary.h beyond tests/test_abi_ledger.py: no entry point takes a size or a 64-bit count; the grid cap is one
    number in the header and in ops."""
    from vnet_tensorflow_amd import ops
    assert not any(p[3] in ("size_t", "long long") for params in guard.header_functions(HEADER).values() for p in params)
    assert ops.SUMMARY_MAX_BLOCKS == 4096 and "#define VNET_SUMMARY_MAX_BLOCKS 4096" in open(HEADER).read()


def test_error_codes_need_no_device():
    """VNET_E_BADARG (-1) for a null pointer or an extent < 1, then VNET_E_UNSUPPORTED (-2) for more than 2^31 - 1 elements: before any
    launch, in that order."""
    from vnet_tensorflow_amd import _lib
    L = _lib.lib()
    one = ctypes.c_void_p(16)
    for name, lead in (("vnet_summary_slices_f32", ()), ("vnet_summary_slices_i32", (63,)), ("vnet_summary_slices_i64", (63,)),
                       ("vnet_summary_rainbow_f32", ())):
        fn = getattr(L, name)
        dims = (2, 5, 7, 3, 3)
        assert fn(None, one, *lead, *dims, None) == -1 and fn(one, None, *lead, *dims, None) == -1
        for pos in range(5):
            for v in (0, -1):
                bad = list(dims)
                bad[pos] = v
                assert fn(one, one, *lead, *bad, None) == -1, (name, pos, v)
        assert fn(one, one, *lead, 1, 2048, 1024, 1024, 1, None) == -2                   # 2^31 elements
        assert fn(one, one, *lead, 2, 1024, 1024, 1024, 1, None) == -2
        assert fn(one, one, *lead, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, None) == -2
        assert fn(None, one, *lead, 1, 2048, 1024, 1024, 1, None) == -1                  # BADARG comes first
        assert fn(one, one, *lead, 1, 2048, 0, 1024, 1024, None) == -1


# ---- config --------------------------------------------------------------------------------------------------------------------------
def _config(**over):
    T = {"Data": {"TrainingDataDirectory": "synthetic", "TestingDataDirectory": "synthetic", "ImageFilenames": ["image.npy"],
                  "LabelFilename": "label.npy"},
         "SegmentationClasses": [0, 1], "BatchSize": 1, "PatchShape": [16, 16, 16],
         "Networks": {"Name": "VNet", "Dropout": 0.0, "NumChannel": 4, "NumLevels": 2, "NumCovolutions": [1, 2], "BottomConvolutions": 1},
         "Loss": {"Name": "sorensen"}, "Optimizer": {"Name": "Adam", "InitialLearningRate": 1e-2, "Decay": {"Factor": 0.99, "Steps": 100}}}
    T.update(over)
    return {"TrainingSetting": T}


def test_summary_interval_key():
    from vnet_tensorflow_amd.model import image2label
    m = image2label(None, _config(), device="cpu", verbose=False)
    m.read_config()
    assert m.summary_interval == 0 and not m._summary_on and m._summary_writers == (None, None)
    for ok in (0, 1, 25):
        m = image2label(None, _config(SummaryInterval=ok), device="cpu", verbose=False)
        m.read_config()
        assert m.summary_interval == ok
    for bad in (-1, 1.0, 2.5, "1", True, None, [1]):
        m = image2label(None, _config(SummaryInterval=bad), device="cpu", verbose=False)
        with pytest.raises(SystemExit, match="SummaryInterval"):
            m.read_config()
    for name in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "SummaryInterval" in open(os.path.join(ROOT, name)).read(), name


def test_every_rank_takes_the_summary_steps_and_rank_0_writes(tmp_path):
    """The rank rule without a process group: which steps are summary steps is read from global_step and the config alone (all ranks
    enqueue them eagerly at the same step); only rank 0 opens event files, and LogDir/test only with Testing."""
    from vnet_tensorflow_amd.model import image2label
    for rank, testing in ((1, True), (0, False), (0, True)):
        log = tmp_path / ("log_%d_%d" % (rank, testing))
        m = image2label(None, _config(SummaryInterval=3, LogDir=str(log), Testing=testing), device="cpu", verbose=False)
        m.read_config()
        m.rank = rank
        assert not m._summary_due()
        m._open_summaries()
        try:
            due = []
            for step in range(7):
                m.global_step = step
                due.append(m._summary_due())
            assert due == [False, False, True, False, False, True, False]          # the steps that END at global step 3 and 6
            train, test = m._summary_writers
            assert (train is not None) == (rank == 0) and (test is not None) == (rank == 0 and testing)
        finally:
            m._close_summaries()
        assert m._summary_writers == (None, None) and not m._summary_due()
        runs = sorted(os.path.relpath(os.path.dirname(f), str(log)) for f in S.event_files(str(log)))
        assert runs == ([] if rank else (["test", "train"] if testing else ["train"]))
