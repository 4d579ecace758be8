"""CPU: the guarded arena of tests/guard.py reports what it must.  The "kernels" here are numpy writing through a CPU arena; nothing
overruns on a GPU on purpose."""
import numpy as np
import pytest
import torch

from tests import guard


def _arena(**kw):
    return guard.Arena("cpu", capacity=24 << 20, **kw)


def _bytes(a):
    return a.buf.numpy()          # (CPU arena: shares memory)


def test_layout_alignment_and_guard_sizes():
    a = _arena()
    x = a.tensor("x", (2, 5, 9, 17, 3), torch.float32, "in", np.arange(2 * 5 * 9 * 17 * 3))
    y = a.tensor("y", (7,), torch.bfloat16, "out")
    ws = a.tensor("ws", (1000,), torch.uint8, "ws")
    for t in (x, y, ws):
        assert t.data_ptr() % 16 == 0 and t.data_ptr() % 32 == 16          # 16-byte aligned, and no more than that
    ex, ey = a.entry("x"), a.entry("y")
    assert ex.back == (ex.off + ex.nbytes, ex.off + ex.nbytes + (1 << 20))      # the back guard starts at the last byte + 1
    assert ex.front[1] == ex.off and ex.off - ex.front[0] >= 1 << 20
    assert ey.front[0] == ex.back[1]
    assert torch.isnan(y.float()).all() and (ws == 0xFF).all()                  # poison: NaN as bf16
    assert torch.isnan(a.buf[ex.back[0]:ex.back[0] + 8].view(torch.float32)).all()
    assert (a.buf[ex.back[0]:ex.back[0] + 8].view(torch.int32) == -1).all()
    big = guard.Arena("cpu", capacity=40, min_guard=16)
    assert big.guard_bytes((1, 4, 64, 64, 32), torch.float32) == 3 * 64 * 64 * 32 * 4      # three z-planes when that is more
    assert a.find(x.data_ptr() + 12).name == "x" and a.find(x.data_ptr() - 1) is None
    a.check()
    with pytest.raises(guard.GuardError, match="full"):
        big.tensor("z", (4,), torch.float32, "out")


def test_reports_one_byte_past_the_end():
    a = _arena()
    a.tensor("y", (2, 3, 4, 5, 6), torch.float32, "out")
    e = a.entry("y")
    _bytes(a)[e.off + e.nbytes] = 0
    with pytest.raises(guard.GuardError) as err:
        a.check()
    msg = str(err.value)
    assert "'y'" in msg and "back guard" in msg and "1 bytes changed" in msg and "+%d" % e.nbytes in msg and "1 .. 1 bytes past its end" in msg


def test_reports_one_byte_before_the_start_and_far_into_a_guard():
    a = _arena()
    a.tensor("pad", (3,), torch.float32, "in", [1, 2, 3])
    a.tensor("stats", (4, 2, 16), torch.float32, "out")
    e = a.entry("stats")
    _bytes(a)[e.off - 1] = 7
    with pytest.raises(guard.GuardError, match=r"'stats'.*front guard.*1 bytes changed.*offset -1.*1 \.\. 1 bytes before its start"):
        a.check()
    _bytes(a)[e.off - 1] = 0xFF
    a.check()
    far = e.back[1] - 5                     # the guard's last bytes, ~1 MiB behind the tensor
    _bytes(a)[far:far + 4] = np.frombuffer(np.float32(1.5).tobytes(), np.uint8)
    with pytest.raises(guard.GuardError) as err:
        a.check()
    assert "back guard" in str(err.value) and "%d .. %d bytes past its end" % ((1 << 20) - 4, (1 << 20) - 1) in str(err.value)


def test_reports_a_modified_input():
    a = _arena()
    x = a.tensor("x", (10,), torch.float32, "in", np.arange(10))
    a.tensor("y", (10,), torch.float32, "out")
    a.check()
    x.numpy()[7] = -1.0
    with pytest.raises(guard.GuardError, match=r"'x'.*input modified.*first at byte offset \+30, last at \+31"):
        a.check()


def test_reports_an_unwritten_output_element():
    a = _arena()
    x = a.tensor("x", (6, 4), torch.float32, "in", np.ones((6, 4)))
    y = a.tensor("y", (6, 4), torch.float32, "out")
    p = a.tensor("pred", (6,), torch.int64, "out")
    y.numpy()[:5] = x.numpy()[:5] * 2        # a "kernel" that forgets the last row
    p.numpy()[:] = 3
    a.check()
    with pytest.raises(guard.GuardError, match=r"'y'.*4 of 24 elements never written.*first at element 20"):
        a.check_written()
    y.numpy()[5] = 2.0
    a.check_written()
    # a written element may hold SOME 0xFF bytes: only an element of nothing but 0xFF counts
    y.numpy().view(np.uint32)[0, 0] = 0xFFFF0000
    a.check_written()


def _leaky_colsum(a):
    """numpy stand-in for a split kernel that ADDS into its partial rows instead of writing them on first touch."""
    x = a.tensor("x", (8, 4), torch.float32, "in", np.arange(32).reshape(8, 4))
    ws = a.tensor("ws", (2, 4), torch.float32, "ws")
    out = a.tensor("out", (4,), torch.float32, "out")
    with np.errstate(invalid="ignore"):
        ws.numpy()[0] += x.numpy()[:4].sum(0)            # the bug: += on scratch nobody initialised
        ws.numpy()[1] = x.numpy()[4:].sum(0)
        out.numpy()[:] = ws.numpy().sum(0)
    return a.snapshot()


def _sound_colsum(a):
    x = a.tensor("x", (8, 4), torch.float32, "in", np.arange(32).reshape(8, 4))
    ws = a.tensor("ws", (2, 4), torch.float32, "ws")
    out = a.tensor("out", (4,), torch.float32, "out")
    ws.numpy()[0] = x.numpy()[:4].sum(0)
    ws.numpy()[1] = x.numpy()[4:].sum(0)
    out.numpy()[:] = ws.numpy().sum(0)
    return a.snapshot()


def test_two_prefills_expose_scratch_that_leaks_into_the_result():
    guard.assert_same_bits(_sound_colsum(_arena()), _sound_colsum(_arena(poison=0)))
    zero = _leaky_colsum(_arena(poison=0))
    assert np.array_equal(zero[0][1].view(np.float32), np.arange(32).reshape(8, 4).sum(0))      # "it was zero when I tested it"
    with pytest.raises(guard.GuardError, match="'out'.*bytes differ between the 0xFF and the 0x00 pre-fill"):
        guard.assert_same_bits(_leaky_colsum(_arena()), zero)


def test_torch_proxy_and_recording_lib_on_the_cpu():
    a = _arena()
    proxy = guard.TorchProxy(a)
    y = proxy.empty((3, 4), dtype=torch.float32, device="cpu")
    z = proxy.zeros(5, dtype=torch.int32, device="cpu")
    o = proxy.ones_like(y)
    e = proxy.empty_like(z)
    assert a.find(y.data_ptr()).role == "out" and a.find(z.data_ptr()).role == "inout" and a.find(e.data_ptr()).role == "out"
    assert torch.isnan(y).all() and (z == 0).all() and (o == 1).all() and (e == -1).all()
    assert proxy.empty(2, device="meta").device.type == "meta" and proxy.float32 is torch.float32
    calls = []

    class Fake(object):
        def vnet_colsum(self, *args):
            return 0

        def vnet_colsum_ws_bytes(self, C):
            return 64
    L = guard.RecordingLib(Fake(), a, calls)
    assert L.vnet_colsum_ws_bytes(4) == 64 and calls == []
    assert L.vnet_colsum(y.data_ptr(), o.data_ptr(), 3, 4, None, 0, None) == 0 and calls == ["vnet_colsum"]
    outside = torch.zeros(4)
    with pytest.raises(guard.GuardError, match="vnet_colsum: argument `out`.*not a tensor of the arena"):
        L.vnet_colsum(y.data_ptr(), outside.data_ptr(), 3, 4, None, 0, None)


def test_header_parser_sees_const_and_pointers():
    fns = guard.header_functions()
    assert [p[0] for p in fns["vnet_colsum"]] == ["x", "out", "M", "C", "ws", "ws_bytes", "stream"]
    assert fns["vnet_colsum"][0][1:3] == (True, True) and fns["vnet_colsum"][1][1:3] == (True, False)
    table = guard.pointer_entry_points()
    assert "vnet_conv_fwd" in table and "vnet_wgrad_flush" not in table and "vnet_set_option" not in table and "vnet_version" not in table
    assert "vnet_conv_ws_bytes" not in table and "vnet_conv_wgrad_b16_group" in table


def test_every_non_const_pointer_of_the_header_is_a_destination():
    """RecordingLib treats an `in` tensor handed to a non-const pointer parameter as a destination (y +=, p -=) and stops checking it
    for changes.  That is sound because every non-const pointer parameter of the header IS an output or accumulate target; a new one
    is added here knowingly."""
    names = set(p[0] for ps in guard.pointer_entry_points().values() for p in ps if guard._is_buffer(p) and not p[2])
    assert names == {
        'CQ', 'G', 'NP', 'acc', 'cbc', 'ceff', 'cm_out', 'coef', 'count', 'dalpha', 'db', 'db1', 'db2', 'db3', 'dbeta', 'deff', 'dg1',
        'dg2', 'dg3', 'dgamma', 'dice_out', 'dlogits', 'doutput', 'ds', 'ds16', 'dw', 'dx', 'dx16', 'hist_out', 'invstd', 'loss_out', 'm',
        'mask', 'mean', 'mm2', 'mm3', 'moving_mean', 'moving_var', 'mv2', 'mv3', 'out', 'p', 'pred_out', 'softmax_out', 'state', 'stats',
        'sums', 'v', 'vol', 'wbc', 'wp', 'ws', 'wv', 'xhat_coef', 'xv', 'y', 'y0', 'y1', 'y16'}
