"""TensorBoard event files without TensorFlow: what the reference's `tf.summary.FileWriter(LogDir + '/train' | '/test')` leaves behind
(model.py:704-709, 754-755, 793-794) -- scalar and image summaries of a step -- written, read back and listed.

An event file is a sequence of TFRecords: `uint64 length | masked_crc32c(length) | data | masked_crc32c(data)`, little endian, the
CRC-32C and its mask those of tf_checkpoint.py.  `data` is a serialised `Event` protobuf, encoded here by hand (event.proto, summary.proto):
    Event          wall_time = 1 (double), step = 2 (int64), file_version = 3 (string), summary = 5 (Summary)
    Summary        value = 1 (repeated Summary.Value)
    Summary.Value  tag = 1 (string), simple_value = 2 (float), image = 4 (Summary.Image)
    Summary.Image  height = 1, width = 2, colorspace = 3 (1 grey, 3 RGB), encoded_image_string = 4 (a PNG)
The first record of a file is Event{wall_time, file_version "brain.Event:2"}; the graph record that FileWriter(..., sess.graph) adds is
not written (there is no GraphDef).  PNGs are 8-bit grey or RGB, non-interlaced, filter type 0, zlib level PNG_LEVEL: the decoded
pixels are TensorFlow's, the bytes are not.  The format is restated from its published definition and pinned by hand-assembled
known-answer bytes and its own round trip (tests/test_summary_host.py): UNPINNED by a real TensorFlow / TensorBoard, like tf_checkpoint.py.

Also here: the NumPy restatements of include/vnet_hip_summary.h (slices_intensity, slices_index, slices_rainbow: float32, operation by
operation -- the yardsticks of tests/test_hip_summary.py), the tag rule of TF 1.15 (step_tags; table in DESIGN.md section 6g) and
`python -m vnet_tensorflow_amd.summary LOGDIR`, which prints the scalars of every event file under LOGDIR as a table."""
import os
import queue
import re
import socket
import struct
import sys
import threading
import time
import zlib

import numpy as np

from .tf_checkpoint import _TABLE, _pb_fields, _put_varint, crc32c, mask_crc

FILE_VERSION = "brain.Event:2"
QUEUE_SIZE = 10          # tf.summary.FileWriter's max_queue
PNG_LEVEL = 1            # zlib level of the image summaries (speed over size: a 128^3 step logs tens of MB of pixels)


# ---- CRC-32C of a large record -----------------------------------------------------------------------------------------------------
_CRC_LANES = 16384
_CRC_TABLE = np.array(_TABLE, dtype=np.uint32)


def crc32c_bulk(data):
    """tf_checkpoint.crc32c(data), for the tens of MB an image summary holds (the byte loop takes seconds there).  The table-driven
    register update is linear over GF(2) in (register, data): the tail of the data is cut into _CRC_LANES segments of equal length
    whose registers advance together, one NumPy step per byte position, beside 32 lanes that carry the basis vectors through the same
    number of zero bytes -- they give the operator "advance by one segment", as four byte tables --; then
    register(A || B) = advance(register(A)) ^ register(B from 0), segment by segment.  Short data take the byte loop."""
    buf = np.frombuffer(data, dtype=np.uint8)
    seg = buf.size // _CRC_LANES
    if seg < 16:
        return crc32c(data)
    head = buf.size - seg * _CRC_LANES
    body = np.ascontiguousarray(buf[head:].reshape(_CRC_LANES, seg).T).astype(np.uint32)
    reg = np.zeros(_CRC_LANES + 32, dtype=np.uint32)
    reg[0] = crc32c(bytes(buf[:head])) ^ 0xffffffff
    reg[_CRC_LANES:] = np.uint32(1) << np.arange(32, dtype=np.uint32)
    low = np.zeros(_CRC_LANES + 32, dtype=np.uint32)
    for j in range(seg):
        low[:_CRC_LANES] = body[j]
        reg = _CRC_TABLE[(reg ^ low) & 0xff] ^ (reg >> 8)
    basis = [int(v) for v in reg[_CRC_LANES:]]
    tabs = []
    for p in range(4):
        t = [0] * 256
        for v in range(1, 256):
            k = v & -v
            t[v] = t[v ^ k] ^ basis[8 * p + k.bit_length() - 1]
        tabs.append(t)
    t0, t1, t2, t3 = tabs
    total = 0
    for r in reg[:_CRC_LANES].tolist():
        total = t0[total & 0xff] ^ t1[(total >> 8) & 0xff] ^ t2[(total >> 16) & 0xff] ^ t3[total >> 24] ^ r
    return total ^ 0xffffffff


# ---- protobuf, the fields an event uses ----------------------------------------------------------------------------------------------
def _key(field, wire):
    return _put_varint(field << 3 | wire)


def _pb_bytes(field, data):
    return _key(field, 2) + _put_varint(len(data)) + bytes(data)


def _pb_varint(field, v):
    return _key(field, 0) + _put_varint(int(v))


def encode_value(tag, value):
    """Summary.Value: value a number (simple_value, rounded to float32) or (height, width, colorspace, png bytes)."""
    out = _pb_bytes(1, tag.encode("utf-8"))
    if isinstance(value, tuple):
        h, w, cs, png = value
        img = _pb_varint(1, h) + _pb_varint(2, w) + _pb_varint(3, cs) + _pb_bytes(4, png)
        return out + _pb_bytes(4, img)
    return out + _key(2, 5) + struct.pack("<f", float(value))


def encode_event(wall_time, step=0, values=None, file_version=None):
    """Event{wall_time, step, file_version | summary}; proto3: a zero step is omitted.  values: [(tag, value)] in order."""
    out = _key(1, 1) + struct.pack("<d", float(wall_time))
    if step:
        out += _pb_varint(2, step)
    if file_version is not None:
        out += _pb_bytes(3, file_version.encode("utf-8"))
    if values is not None:
        out += _pb_bytes(5, b"".join(_pb_bytes(1, encode_value(t, v)) for t, v in values))
    return out


def encode_record(data):
    """One TFRecord around `data`."""
    head = struct.pack("<Q", len(data))
    return head + struct.pack("<I", mask_crc(crc32c(head))) + bytes(data) + struct.pack("<I", mask_crc(crc32c_bulk(data)))


def read_records(path):
    """The payload of every record of an event file, both CRCs of each verified; ValueError on a damaged or truncated record."""
    with open(path, "rb") as f:
        buf = f.read()
    pos = 0
    while pos < len(buf):
        if pos + 12 > len(buf):
            raise ValueError("%s: truncated record header at byte %d" % (path, pos))
        head = buf[pos:pos + 8]
        n, = struct.unpack("<Q", head)
        if struct.unpack_from("<I", buf, pos + 8)[0] != mask_crc(crc32c(head)):
            raise ValueError("%s: length CRC mismatch at byte %d" % (path, pos))
        if pos + 12 + n + 4 > len(buf):
            raise ValueError("%s: record at byte %d runs past the end of the file" % (path, pos))
        data = buf[pos + 12:pos + 12 + n]
        if struct.unpack_from("<I", buf, pos + 12 + n)[0] != mask_crc(crc32c_bulk(data)):
            raise ValueError("%s: data CRC mismatch in the record at byte %d" % (path, pos))
        yield data
        pos += 16 + n


def parse_event(data):
    """{'wall_time', 'step', 'file_version' (or None), 'values': [(tag, float | (height, width, colorspace, png bytes))]}."""
    ev = {"wall_time": 0.0, "step": 0, "file_version": None, "values": []}
    for f, wt, v in _pb_fields(data):
        if f == 1 and wt == 1:
            ev["wall_time"] = struct.unpack("<d", struct.pack("<Q", v))[0]
        elif f == 2 and wt == 0:
            ev["step"] = v - (1 << 64) if v >> 63 else v
        elif f == 3 and wt == 2:
            ev["file_version"] = v.decode("utf-8")
        elif f == 5 and wt == 2:
            for f1, wt1, val in _pb_fields(v):
                if f1 != 1 or wt1 != 2:
                    continue
                tag, content = "", None
                for f2, wt2, x in _pb_fields(val):
                    if f2 == 1 and wt2 == 2:
                        tag = x.decode("utf-8")
                    elif f2 == 2 and wt2 == 5:
                        content = struct.unpack("<f", struct.pack("<I", x))[0]
                    elif f2 == 4 and wt2 == 2:
                        img = {1: 0, 2: 0, 3: 0, 4: b""}
                        for f3, _wt3, y in _pb_fields(x):
                            img[f3] = y
                        content = (img[1], img[2], img[3], img[4])
                ev["values"].append((tag, content))
    return ev


def read_events(path):
    """Yields (wall_time, step, {tag: float | (height, width, colorspace, png bytes)}) for every record of an event file (the version
    record first, with an empty dict); dicts keep the order the values were written in.  Both CRCs of every record are verified."""
    for data in read_records(path):
        ev = parse_event(data)
        yield ev["wall_time"], ev["step"], dict(ev["values"])


def file_version(path):
    """file_version of the first record ("brain.Event:2")."""
    for data in read_records(path):
        return parse_event(data)["file_version"]
    return None


# ---- PNG -----------------------------------------------------------------------------------------------------------------------------
def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xffffffff)


def encode_png(pixels, level=PNG_LEVEL):
    """uint8 [H, W] (grey) or [H, W, 3] (RGB) -> PNG bytes: bit depth 8, non-interlaced, every row filter type 0."""
    a = np.ascontiguousarray(pixels)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3) or a.size == 0:
        raise ValueError("encode_png: takes uint8 [H, W] or [H, W, 3], got %s %s" % (a.dtype, a.shape))
    h, w = a.shape[:2]
    rows = np.zeros((h, 1 + a.size // h), dtype=np.uint8)
    rows[:, 1:] = a.reshape(h, -1)
    ihdr = struct.pack(">IIBBBBB", w, h, 8, 0 if a.ndim == 2 else 2, 0, 0, 0)
    return b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(rows.tobytes(), level)) + _chunk(b"IEND", b"")


def image_value(pixels):
    """Summary.Image of a uint8 array [H, W] or [H, W, 3]: (height, width, colorspace, png bytes)."""
    a = np.asarray(pixels)
    return int(a.shape[0]), int(a.shape[1]), 1 if a.ndim == 2 else 3, encode_png(a)


# ---- the writer ----------------------------------------------------------------------------------------------------------------------
class FileWriter(object):
    """tf.summary.FileWriter(logdir): `events.out.tfevents.<unix seconds, 10 digits>.<hostname>` in `logdir` (created; a file of that
    name already there -- a restart within the same second -- gets a numeric suffix, older files stay).

    add_summary(values, step, wait=None) queues one Event; values: [(tag, v)] with v a number, a uint8 array [H, W] / [H, W, 3] (PNG-
    encoded by the worker), a ready (height, width, colorspace, png bytes), or a callable returning one of these (called by the worker).
    wait: an object whose .synchronize() the worker calls first (the event behind the device-to-host copy the arrays are views of).
    ONE worker thread per writer encodes and writes.  The queue holds QUEUE_SIZE events and add_summary BLOCKS while it is full:
    nothing is dropped.  An exception in the worker is re-raised by the next add_summary / flush / close on the caller's thread (the
    events queued behind the failing one are discarded).  close() drains the queue and is idempotent."""

    def __init__(self, logdir, max_queue=QUEUE_SIZE, filename_suffix=""):
        os.makedirs(logdir, exist_ok=True)
        base = os.path.join(logdir, "events.out.tfevents.%010d.%s%s" % (int(time.time()), socket.gethostname(), filename_suffix))
        path, k = base, 0
        while os.path.exists(path):
            k += 1
            path = "%s.%d" % (base, k)
        self.path = path
        self._file = open(path, "wb")
        self._file.write(encode_record(encode_event(time.time(), file_version=FILE_VERSION)))
        self._file.flush()
        self._queue = queue.Queue(maxsize=int(max_queue))
        self._error = None
        self._closed = False
        self._thread = threading.Thread(target=self._work, name="summary-writer", daemon=True)
        self._thread.start()

    # worker -----------------------------------------------------------------------------------------------------------
    @staticmethod
    def _resolve(v):
        if callable(v):
            v = v()
        if isinstance(v, np.ndarray):
            return image_value(v)
        return v

    def _work(self):
        while True:
            item = self._queue.get()
            try:
                if item is None:
                    return
                if isinstance(item, threading.Event):
                    if self._error is None:
                        self._file.flush()
                    item.set()
                    continue
                if self._error is not None:
                    continue
                wall_time, step, values, wait = item
                if wait is not None:
                    wait.synchronize()
                self._file.write(encode_record(encode_event(wall_time, step, [(t, self._resolve(v)) for t, v in values])))
                self._file.flush()            # (the reference flushes after every add_summary)
            except BaseException as e:        # surfaces on the caller's thread
                self._error = e
            finally:
                self._queue.task_done()

    def _raise(self):
        if self._error is not None:
            e, self._error = self._error, None
            raise e

    # caller -----------------------------------------------------------------------------------------------------------
    def add_summary(self, values, step, wait=None):
        self._raise()
        if self._closed:
            raise ValueError("add_summary on a closed FileWriter (%s)" % self.path)
        self._queue.put((time.time(), int(step), list(values), wait))

    def flush(self):
        """Returns once every event queued so far is in the file."""
        if not self._closed:
            done = threading.Event()
            self._queue.put(done)
            done.wait()
        self._raise()

    def close(self):
        if not self._closed:
            self._closed = True
            self._queue.put(None)
            self._thread.join()
            self._file.close()
        self._raise()


# ---- tags (TF 1.15) ------------------------------------------------------------------------------------------------------------------
def clean_tag(name):
    """summary_op_util.clean_tag: characters outside [-/\\w.] become '_', leading slashes go."""
    return re.sub(r"[^-/\w\.]", "_", name).lstrip("/")


def image_tags(name, n):
    """tf.summary.image(name, t, max_outputs=n) on a batch of n images: name/image/0 .. name/image/(n-1); name/image for n == 1."""
    name = clean_tag(name)
    return ["%s/image" % name] if n == 1 else ["%s/image/%d" % (name, i) for i in range(n)]


def is_mixed(loss_name):
    return loss_name.startswith("mixed_")


def scalar_names(label_classes, loss_name):
    """{what: tag} of the scalars of a step.  A scalar's tag is its enclosing name scopes plus its cleaned name; `learning_rate` is
    written outside of the scope `learning_rate` that the schedule was built in (model.py:641-644), so its summary op -- and with it
    the tag -- is uniquified to `learning_rate_1`."""
    tags = {}
    if is_mixed(loss_name):
        tags["dice"] = "loss/1.dice"
        tags["xent"] = "loss/2.regularized_xent"
    tags["loss"] = "loss/0.total_loss"
    tags["accuracy"] = "metrics/accuracy"
    for c in list(label_classes)[1:]:
        for what in ("sensitivity", "specificity", "dice", "auc"):
            tags[(what, c)] = "metrics/" + clean_tag("%s_%s" % (what, c))
    tags["learning_rate"] = "learning_rate_1"
    return tags


def step_tags(image_filenames, label_classes, batch_size, depth, loss_name, image_log):
    """Every tag of one merged summary, in the order the reference's graph creates them (tf.summary.merge_all keeps it): input
    channels and label per batch item, rainbow softmax per batch item and class, the loss scalars, the prediction, the metrics, the
    learning rate."""
    names = scalar_names(label_classes, loss_name)
    out = []
    if image_log:
        for b in range(batch_size):
            for f in image_filenames:
                out += image_tags("%s_batch%d" % (f, b), depth)
            out += image_tags("label_batch%d" % b, depth)
        for b in range(batch_size):
            for c in label_classes:
                out += image_tags("softmax_%s_batch%d" % (c, b), depth)
    out += [names[k] for k in ("dice", "xent", "loss") if k in names]
    if image_log:
        for b in range(batch_size):
            out += image_tags("pred_batch%d" % b, depth)
    out += [t for k, t in names.items() if k == "accuracy" or isinstance(k, tuple)]
    out.append(names["learning_rate"])
    return out


# ---- NumPy restatements of include/vnet_hip_summary.h --------------------------------------------------------------------------------
def index_factor(num_classes, label_classes):
    """The grey level step of the label / prediction images (model.py:330-333, 580-583)."""
    k = int(num_classes) - 1 if 0 in list(label_classes) else int(num_classes)
    if k < 1:
        raise ValueError("index_factor: %d classes with class 0 among them leave nothing to scale" % num_classes)
    return 255 // k


def _bytes_of(v):
    """tf.cast(float32 -> uint8) where it is defined (truncation); v <= -1 -> 0, v >= 256 -> 255, NaN -> 0: this project's choice."""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        inside = np.where(v > 0, np.minimum(v, np.float32(255)), np.float32(0))
    return np.trunc(inside).astype(np.uint8)


def _planes(a):
    """[B,X,Y,Z,C, ...] -> [B,C,Z,X,Y, ...]: plane [b][c][z] = tf.transpose(t[b:b+1, :, :, :, c], [3,1,2,0])[z]."""
    return np.ascontiguousarray(np.moveaxis(np.moveaxis(a, 4, 1), 4, 2))


def slices_intensity(images):
    """vnet_summary_slices_f32: float32 [B,X,Y,Z,C] -> uint8 [B,C,Z,X,Y]."""
    return _planes(_bytes_of(images))


def slices_index(index, factor):
    """vnet_summary_slices_i32 / _i64: integer [B,X,Y,Z,C] -> uint8 [B,C,Z,X,Y] = (index * factor) mod 256."""
    with np.errstate(over="ignore"):
        prod = np.asarray(index).astype(np.int64) * np.int64(factor)
    return _planes((prod & 255).astype(np.uint8))


def rainbow(p):
    """grayscale_to_rainbow (model.py:16-24) with tf.image.hsv_to_rgb at S = V = 1, times 255, cast: float32 [...] -> uint8 [..., 3].
    Every line is one float32 operation."""
    p = np.asarray(p, dtype=np.float32)
    one, two, three, four, six = (np.float32(v) for v in (1, 2, 3, 4, 6))
    with np.errstate(invalid="ignore"):
        h = one - p
        h = h * two
        h = h / three
        dh = h * six
        r = np.clip(np.abs(dh - three) - one, np.float32(0), one)
        g = np.clip(two - np.abs(dh - two), np.float32(0), one)
        b = np.clip(two - np.abs(dh - four), np.float32(0), one)
        rgb = np.stack([r, g, b], axis=-1) * np.float32(255)
    assert rgb.dtype == np.float32
    return _bytes_of(rgb)


def slices_rainbow(softmax):
    """vnet_summary_rainbow_f32: float32 [B,X,Y,Z,K] -> uint8 [B,K,Z,X,Y,3]."""
    return _planes(rainbow(softmax))


# ---- python -m vnet_tensorflow_amd.summary LOGDIR -----------------------------------------------------------------------------------
def event_files(logdir):
    out = []
    for root, _dirs, files in os.walk(logdir):
        out += [os.path.join(root, f) for f in files if f.startswith("events.out.tfevents.")]
    return sorted(out)


def scalar_table(logdir):
    """[(run directory relative to logdir, step, {tag: float})] over every event file under logdir, in file then record order."""
    rows = []
    for path in event_files(logdir):
        run = os.path.relpath(os.path.dirname(path), logdir)
        for _wall, step, values in read_events(path):
            scalars = {t: v for t, v in values.items() if isinstance(v, float)}
            if scalars:
                rows.append((run, step, scalars))
    return rows


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) != 1:
        print("usage: python -m vnet_tensorflow_amd.summary LOGDIR", file=sys.stderr)
        return 2
    rows = scalar_table(argv[0])
    tags = []
    for _run, _step, scalars in rows:
        tags += [t for t in scalars if t not in tags]
    widths = [max(12, len(t)) for t in tags]
    print("%-8s %8s  %s" % ("run", "step", "  ".join("%*s" % (w, t) for w, t in zip(widths, tags))))
    for run, step, scalars in rows:
        print("%-8s %8d  %s" % (run, step, "  ".join(
            "%*s" % (w, ("%.6g" % scalars[t]) if t in scalars else "-") for w, t in zip(widths, tags))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
