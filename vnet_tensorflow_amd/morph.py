"""The device ops over csrc/vnet_tools.h (csrc/morph.hip): the bit-packed morphology the data-preparation tools run on the device
(vnet_tensorflow_amd/prepare_data.py).  The header is the package's own, not part of the published C ABI; its
entry points live in libvnet_hip.so and are bound by _lib.lib() like every other row of _lib.HEADERS.

Same conventions as _lib / ops: there is NO fallback -- a missing library or a kernel that reports an error raises VnetHipError,
nothing routes to PyTorch or the CPU; ops launch on torch's current stream of the calling thread; outputs are allocated through this
module's `torch` name.

Every op takes a dense 3-D device tensor [A,B,C] and gives the axes no meaning.  A PACKED MASK is an int64 tensor [A,B,ceil(C/64)]:
bit k of word w is voxel c = 64 w + k, the unused high bits of a row's last word are zero.  The word count loses C, so the ops that
take a mask take C beside it."""
import ctypes

import torch

from ._lib import VnetHipError, check, lib
from .ops import _thread_stream as _stream

HEADER = "vnet_tensorflow_amd/csrc/vnet_tools.h"          # its row of _lib.HEADERS

MAX_VALUES, MAX_RADIUS, MAX_VOXELS = 16, 8, 2 ** 31 - 1
# dtype_code of vnet_select_bits
DTYPE_CODES = {torch.uint8: 0, torch.int8: 1, torch.int16: 2, torch.uint16: 3, torch.int32: 4}
_RANGES = {0: (0, 255), 1: (-128, 127), 2: (-32768, 32767), 3: (0, 65535), 4: (-2 ** 31, 2 ** 31 - 1)}


def words(C):
    return (int(C) + 63) // 64


def _volume(x, what):
    """(A, B, C) of a dense 3-D device tensor."""
    if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.numel() == 0:
        raise VnetHipError("%s: takes a non-empty [A,B,C] tensor, got %s" % (what, tuple(getattr(x, "shape", ())) or type(x).__name__))
    if x.device.type != "cuda":
        raise VnetHipError("%s: the tensor is on %s; the kernels run on the device only (no CPU path)" % (what, x.device))
    if x.numel() > MAX_VOXELS:
        raise VnetHipError("%s: %dx%dx%d has more voxels than an int32 indexes" % ((what,) + tuple(x.shape)))
    return tuple(int(v) for v in x.shape)


def _mask(bits, C, what):
    """(A, B, C) of a packed mask with C voxels per row."""
    A, B, W = _volume(bits, what)
    C = int(C)
    if bits.dtype != torch.int64:
        raise VnetHipError("%s: a packed mask is int64, got %s" % (what, bits.dtype))
    if C < 1 or W != words(C):
        raise ValueError("%s: a mask of %d words per row does not hold rows of C = %d voxels" % (what, W, C))
    if A * B * C > MAX_VOXELS:
        raise VnetHipError("%s: %dx%dx%d has more voxels than an int32 indexes" % (what, A, B, C))
    return A, B, C


def select_bits(label, values, dtype_code=None):
    """uint8 / int8 / int16 / uint16 / int32 device tensor [A,B,C] -> the packed mask of `label in values` (prepare_data.select):
    1 .. 16 distinct integers, each inside the dtype's range.  dtype_code overrides the tensor's dtype among those of its width."""
    A, B, C = _volume(label, "select_bits")
    code = DTYPE_CODES.get(label.dtype) if dtype_code is None else int(dtype_code)
    if code not in _RANGES or label.element_size() != (1, 1, 2, 2, 4)[code]:
        raise VnetHipError("select_bits: expected uint8, int8, int16, uint16 or int32, got %s (code %r)" % (label.dtype, dtype_code))
    values = [int(v) for v in values]
    if len(set(values)) != len(values):
        raise ValueError("select_bits: values %r are not distinct" % (values,))
    if not 1 <= len(values) <= MAX_VALUES:
        raise ValueError("select_bits: takes 1 .. %d values, got %d" % (MAX_VALUES, len(values)))
    lo, hi = _RANGES[code]
    if any(v < lo or v > hi for v in values):
        raise ValueError("select_bits: values %r outside the label's range %d .. %d" % (values, lo, hi))
    label = label.contiguous()
    bits = torch.empty((A, B, words(C)), dtype=torch.int64, device=label.device)
    host = (ctypes.c_longlong * len(values))(*values)
    with torch.cuda.device(label.device):
        check(lib().vnet_select_bits(label.data_ptr(), code, host, len(values), bits.data_ptr(), A, B, C, _stream(label.device)),
              "vnet_select_bits")
    return bits


def dilate_bits(bits, C, r):
    """Packed mask [A,B,W] of rows of C voxels -> a new packed mask, dilated by ball(r), 1 <= r <= 8 (prepare_data.dilate)."""
    A, B, C = _mask(bits, C, "dilate_bits")
    r = int(r)
    if not 1 <= r <= MAX_RADIUS:
        raise ValueError("dilate_bits: radius %d (1 .. %d)" % (r, MAX_RADIUS))
    bits = bits.contiguous()
    out = torch.empty((A, B, words(C)), dtype=torch.int64, device=bits.device)
    with torch.cuda.device(bits.device):
        check(lib().vnet_dilate_bits(bits.data_ptr(), out.data_ptr(), A, B, C, r, _stream(bits.device)), "vnet_dilate_bits")
    return out


def bits_bbox(bits, C):
    """(count, lo, hi) of a packed mask: lo / hi the inclusive corners (a, b, c) of the box around its set voxels, both None when
    count is 0 (prepare_data.bounding_box).  One read-back of seven numbers."""
    A, B, C = _mask(bits, C, "bits_bbox")
    bits = bits.contiguous()
    out7 = torch.empty(7, dtype=torch.int64, device=bits.device)
    with torch.cuda.device(bits.device):
        check(lib().vnet_bits_bbox(bits.data_ptr(), out7.data_ptr(), A, B, C, _stream(bits.device)), "vnet_bits_bbox")
    row = [int(v) for v in out7.cpu().tolist()]
    if row[0] == 0:
        return 0, None, None
    return row[0], tuple(row[1:4]), tuple(row[4:7])


def masked_crop(src, bits, start, size):
    """Device tensor [A,B,C] of 1-, 2-, 4- or 8-byte elements -> the window [size] at `start`, bit for bit, zeroed where the packed
    mask `bits` (over the whole volume) is 0; bits None: the plain crop.  The window lies inside the volume."""
    A, B, C = _volume(src, "masked_crop")
    eb = src.element_size()
    if eb not in (1, 2, 4, 8) or src.is_complex():
        raise VnetHipError("masked_crop: elements of 1, 2, 4 or 8 bytes, got %s" % (src.dtype,))
    start, size = tuple(int(v) for v in start), tuple(int(v) for v in size)
    if len(start) != 3 or len(size) != 3:
        raise ValueError("masked_crop: start %r and size %r are not three numbers each" % (start, size))
    if any(s < 0 or n < 1 or s + n > e for s, n, e in zip(start, size, (A, B, C))):
        raise ValueError("masked_crop: window start %r size %r does not lie inside %r" % (start, size, (A, B, C)))
    if bits is not None:
        if _mask(bits, C, "masked_crop")[:2] != (A, B) or bits.device != src.device:
            raise ValueError("masked_crop: the mask %s does not cover the volume %s" % (tuple(bits.shape), (A, B, C)))
        bits = bits.contiguous()
    src = src.contiguous()
    dst = torch.empty(size, dtype=src.dtype, device=src.device)
    with torch.cuda.device(src.device):
        check(lib().vnet_masked_crop(src.data_ptr(), None if bits is None else bits.data_ptr(), dst.data_ptr(), A, B, C, eb,
                                     *(start + size), _stream(src.device)), "vnet_masked_crop")
    return dst


def unpack_bits(bits, C):
    """Packed mask [A,B,W] of rows of C voxels -> uint8 [A,B,C] of 0 / 1."""
    A, B, C = _mask(bits, C, "unpack_bits")
    bits = bits.contiguous()
    dst = torch.empty((A, B, C), dtype=torch.uint8, device=bits.device)
    with torch.cuda.device(bits.device):
        check(lib().vnet_unpack_bits(bits.data_ptr(), dst.data_ptr(), A, B, C, _stream(bits.device)), "vnet_unpack_bits")
    return dst
