"""The ledger of the library's C ABI, one row per header of _lib.HEADERS (no GPU; needs the built library).  For every header: the
names it declares are the names its table binds and the literal set written here; every name is exported; every argument and the
result are bound with the ctypes type the declared type has (RULE below: one ctypes type per C type, for every parameter of every
function); every function that takes a buffer ends in `stream` and is named by a case of the header's guard file; the Makefile and
profiles/check_isa.sh name its translation unit.  Across headers: no name declared or bound twice, include/ holds exactly the
registry's published headers, and the size queries lib() memoises are the set it memoised before there was a rule for them plus
the ones written down since.  What only one header has to say stays in that header's tests/test_*_host.py."""
import ctypes
import importlib
import os
import re

import pytest

from tests import guard
from vnet_tensorflow_amd import _lib

ROOT = guard.ROOT
RULE = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "long long": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
        "unsigned long long": ctypes.c_uint64, "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double,
        "const char*": ctypes.c_char_p}
# the two result ints of vnet_packed_dims are the only typed pointers of the binding; every other pointer is a c_void_p
TYPED_POINTERS = {("vnet_packed_dims", "CQ"): ctypes.POINTER(ctypes.c_int), ("vnet_packed_dims", "NP"): ctypes.POINTER(ctypes.c_int)}

VNET_HIP = set("""
vnet_version vnet_set_option vnet_get_option vnet_packed_weight_floats vnet_pack_weights vnet_packed_dims
vnet_pack_weights_batched vnet_conv_ws_bytes vnet_conv_fwd vnet_conv_fwd_acc vnet_conv_stats_rows vnet_conv_stats_from_reduce
vnet_conv_fwd_stats vnet_conv_x3_ok vnet_conv_x3_stats_rows vnet_conv_x3_ws_bytes vnet_conv_fwd_x3 vnet_wgrad_x3_ok
vnet_wgrad_x3_ws_bytes vnet_conv_wgrad_x3 vnet_wgrad_bf16_ws_bytes vnet_wgrad_defer vnet_wgrad_pending vnet_wgrad_flush
vnet_wgrad_ws_bytes vnet_conv_wgrad vnet_tile_im2col_x vnet_input_conv_fold vnet_input_conv_grads vnet_input_conv_direct_ok
vnet_input_conv_direct_stats_rows vnet_input_conv_fold_border vnet_input_conv_direct_fwd vnet_input_wgrad_direct_slabs
vnet_input_wgrad_direct vnet_head_fwd vnet_head_bwd vnet_head_ws_bytes vnet_colsum_ws_bytes vnet_colsum vnet_bn_ws_bytes
vnet_bn_stats vnet_bn_act_fwd vnet_bn_act_bwd vnet_bn_finalize_partial vnet_bn_moments vnet_bn_finalize
vnet_bn_act_bwd_reduce vnet_bn_act_bwd_apply vnet_bn_chain_coef_fwd vnet_bn_chain_coef_bwd vnet_act_fwd vnet_act_bwd
vnet_loss_ws_bytes vnet_softmax_dice_fwd vnet_softmax_dice_bwd vnet_dice_coe_fwd vnet_dice_coe_bwd vnet_dropout_fwd
vnet_dropout_bwd vnet_adam_apply vnet_sgd_apply vnet_momentum_apply vnet_step_state_set vnet_adam_apply_dev
vnet_sgd_apply_dev vnet_momentum_apply_dev vnet_dropout_fwd_dev vnet_confusion_ws_bytes vnet_confusion_matrix
vnet_auc_ws_bytes vnet_auc_histogram vnet_accumulate_patch vnet_cast_bf16 vnet_colsum_b16_ws_bytes vnet_colsum_b16
vnet_conv_b16_ws_bytes vnet_conv_b16_stats_rows vnet_conv_fwd_b16 vnet_conv_fwd_b16_padded vnet_conv_wgrad_b16
vnet_wgrad_job_bytes vnet_conv_wgrad_b16_group vnet_conv2_fwd_b16 vnet_conv2_wgrad_b16 vnet_conv2_direct_ok
vnet_conv2_direct_stats_rows vnet_conv2_direct_b16 vnet_conv2_direct_f32 vnet_bn_stats_b16 vnet_bn_moments_b16
vnet_bn_act_fwd_b16 vnet_bn_act_bwd_reduce_b16 vnet_bn_act_bwd_apply_b16 vnet_bn_small_ok vnet_bn_small_fwd_b16
vnet_bn_small_bwd_b16 vnet_head_fwd_b16 vnet_head_bwd_b16 vnet_dropout_fwd_b16 vnet_dropout_bwd_b16""".split())

# header -> (guard module of tests/, exact name set, the names of it that take NO buffer (None: not pinned for this header),
#            what the Makefile must name, the spellings under which profiles/check_isa.sh names the unit)
LEDGER = {
    "include/vnet_hip.h": (
        "test_hip_guard_bands", VNET_HIP, None,
        ("../../include/vnet_hip.h", " conv_mfma.hip", " conv_x3.hip", " conv_b16.hip", " conv2_b16.hip", " elementwise.hip",
         " input_block.hip"), (" conv_mfma ", " conv_x3 ", " conv_b16 ", " conv2_b16 ", " elementwise ", " input_block ")),
    "include/vnet_hip_unet.h": (
        "test_hip_unet_guard", {"vnet_maxpool2_fwd", "vnet_maxpool2_bwd"}, set(),
        ("../../include/vnet_hip_unet.h", " pool.hip"), (" pool ",)),
    "include/vnet_hip_head.h": (
        "test_hip_head_guard", {"vnet_bn_head_ok", "vnet_bn_head_stats_rows", "vnet_bn_head_ws_bytes", "vnet_bn_act_head_fwd",
                                "vnet_bn_act_bwd_reduce_head", "vnet_bn_act_bwd_apply_head"},
        {"vnet_bn_head_ok", "vnet_bn_head_stats_rows", "vnet_bn_head_ws_bytes"}, ("../../include/vnet_hip_head.h",), ()),
    "include/vnet_hip_resample.h": (
        "test_hip_resample_guard", {"vnet_resample_linear", "vnet_resample_nearest_i32"}, set(),
        ("../../include/vnet_hip_resample.h", " resample.hip"), (" resample ",)),
    "include/vnet_hip_components.h": (
        "test_hip_components_guard", {"vnet_cc_ws_bytes", "vnet_cc_roots", "vnet_cc_largest", "vnet_cc_volume_threshold"},
        {"vnet_cc_ws_bytes"}, ("../../include/vnet_hip_components.h", " components.hip"), (" components ",)),
    "include/vnet_hip_deform.h": (
        "test_hip_deform_guard", {"vnet_bspline_deform_f32", "vnet_bspline_deform_i32"}, set(),
        ("../../include/vnet_hip_deform.h", " deform.hip"), (" deform;",)),
    "include/vnet_hip_sample.h": (
        "test_hip_sample_guard", {"vnet_cc_table_ws_bytes", "vnet_cc_table", "vnet_window_count", "vnet_sample_patch"},
        {"vnet_cc_table_ws_bytes"}, ("../../include/vnet_hip_sample.h", " sample.hip"), (" sample ",)),
    "include/vnet_hip_prepare.h": (
        "test_hip_prepare_guard", {"vnet_channel_stats_ws_bytes", "vnet_channel_stats", "vnet_window_intensity", "vnet_crop_words",
                                   "vnet_argmax_label"},
        {"vnet_channel_stats_ws_bytes"}, ("../../include/vnet_hip_prepare.h", " prepare.hip"), (" prepare ",)),
    "include/vnet_hip_score.h": (
        "test_hip_score_guard", {"vnet_label_overlap", "vnet_cc_shape_ws_bytes", "vnet_cc_shape"}, {"vnet_cc_shape_ws_bytes"},
        ("../../include/vnet_hip_score.h", " score.hip", " cc_table.h"), (" score ",)),
    "include/vnet_hip_summary.h": (
        "test_hip_summary_guard", {"vnet_summary_slices_f32", "vnet_summary_slices_i32", "vnet_summary_slices_i64",
                                   "vnet_summary_rainbow_f32"}, set(),
        ("../../include/vnet_hip_summary.h", " summary.hip"), (" summary ",)),
    "include/vnet_hip_deform_sample.h": (
        "test_hip_deform_sample_guard", {"vnet_deform_sample_patch"}, set(),
        ("../../include/vnet_hip_deform_sample.h", " deform_sample.hip", " bspline_field.h", " philox_noise.h"), (" deform_sample;",)),
    "vnet_tensorflow_amd/csrc/vnet_bbox.h": (
        "test_hip_bbox_guard", {"vnet_slice_stack_f32", "vnet_slice_stack_i32", "vnet_plane_cc_table_ws_bytes", "vnet_plane_cc_table",
                                "vnet_bbox_render"},
        {"vnet_plane_cc_table_ws_bytes"}, (" vnet_bbox.h", " bbox.hip", " cc_union.h", " cc_table.h"), (" bbox;",)),
    "vnet_tensorflow_amd/csrc/vnet_tools.h": (
        "test_hip_prepare_data_guard", {"vnet_select_bits", "vnet_dilate_bits", "vnet_bits_bbox", "vnet_masked_crop",
                                        "vnet_unpack_bits"}, set(), (" vnet_tools.h", " morph.hip"), (" morph;",)),
    "vnet_tensorflow_amd/csrc/vnet_surface.h": (
        "test_hip_surface_guard", {"vnet_surface_bits", "vnet_edt2_ws_bytes", "vnet_edt2", "vnet_surface_gather_ws_bytes",
                                   "vnet_surface_gather", "vnet_list_select_ws_bytes", "vnet_list_select",
                                   "vnet_list_root_sum_ws_bytes", "vnet_list_root_sum"},
        {"vnet_edt2_ws_bytes", "vnet_surface_gather_ws_bytes", "vnet_list_select_ws_bytes", "vnet_list_root_sum_ws_bytes"},
        (" vnet_surface.h", " surface.hip"), (" surface;",)),
}

# what lib() answered from a dict before the rule (_lib.memoised) replaced the two hand-kept lists: written down from that binding
MEMOISED = {
    "vnet_packed_weight_floats", "vnet_conv_x3_stats_rows", "vnet_conv_x3_ws_bytes", "vnet_wgrad_x3_ws_bytes", "vnet_conv_ws_bytes",
    "vnet_conv_stats_rows", "vnet_conv_stats_from_reduce", "vnet_colsum_b16_ws_bytes", "vnet_conv_b16_ws_bytes",
    "vnet_conv_b16_stats_rows", "vnet_wgrad_bf16_ws_bytes", "vnet_wgrad_ws_bytes", "vnet_input_conv_direct_stats_rows",
    "vnet_head_ws_bytes", "vnet_colsum_ws_bytes", "vnet_bn_ws_bytes", "vnet_loss_ws_bytes", "vnet_confusion_ws_bytes",
    "vnet_auc_ws_bytes", "vnet_conv2_direct_stats_rows",
    "vnet_bn_head_ok", "vnet_bn_head_stats_rows", "vnet_bn_head_ws_bytes", "vnet_cc_ws_bytes", "vnet_cc_table_ws_bytes",
    "vnet_channel_stats_ws_bytes", "vnet_cc_shape_ws_bytes", "vnet_plane_cc_table_ws_bytes"}
# what the rule has taken in since: the size queries of csrc/vnet_surface.h (pure in their arguments; they read no option)
MEMOISED_SINCE = {"vnet_edt2_ws_bytes", "vnet_surface_gather_ws_bytes", "vnet_list_select_ws_bytes", "vnet_list_root_sum_ws_bytes"}


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def _ctype(fn_name, param):
    pname, ptr, _const, typ = param
    if ptr and typ.replace(" ", "") != "constchar*":
        return TYPED_POINTERS.get((fn_name, pname), ctypes.c_void_p)
    return RULE[typ]


def _result_types(path):
    """{name: declared result type} of a header ('int', 'size_t', 'double', 'const char*')."""
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    return {m.group(2): " ".join(m.group(1).split()).replace(" *", "*")
            for m in re.finditer(r"^[ \t]*((?:\w+[ \t*]+)+)(vnet_[a-z0-9_]+)[ \t]*\(", text, re.M)}


@pytest.mark.parametrize("header", [h for h, _ in _lib.HEADERS])
def test_header_ledger(header):
    table = dict(_lib.HEADERS)[header]
    module, names, no_buffer, mk_strings, isa_strings = LEDGER[header]
    path = os.path.join(ROOT, header)
    fns = guard.header_functions(path)
    assert set(fns) == set(table) == names, (set(fns) ^ set(table), set(fns) ^ names)
    results = _result_types(path)
    assert set(results) == names
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name, params in fns.items():
        assert hasattr(L, name), name
        res, args = table[name]
        assert len(args) == len(params), name
        for a, p in zip(args, params):
            assert a is _ctype(name, p), (name, p, a)
        assert res is RULE[results[name]], (name, results[name], res)
        assert res is ctypes.c_size_t or not name.endswith("_ws_bytes"), name
    pointer = guard.pointer_entry_points(path)
    if no_buffer is not None:
        assert set(pointer) == names - no_buffer
    covered = set()
    for row in importlib.import_module("tests." + module).CASES.values():
        covered |= set(row[0])
    for name, params in pointer.items():
        device = [p for p in params if guard._is_buffer(p) and (name, p[0]) not in guard.HOST_POINTERS]
        assert params[-1][0] == "stream" or not device, name          # (vnet_packed_dims fills two host ints and launches nothing)
        assert name in covered, "%s: no case of tests/%s.py names it" % (name, module)
    mk, isa = _read("vnet_tensorflow_amd", "csrc", "Makefile"), _read("profiles", "check_isa.sh")
    assert [s for s in mk_strings if s not in mk] == [] and [s for s in isa_strings if s not in isa] == []


def test_ledger_has_a_row_for_every_header_and_include_holds_the_published_ones():
    assert [h for h, _ in _lib.HEADERS] == list(LEDGER) and len(LEDGER) == 14
    assert _lib.HEADERS[0] == ("include/vnet_hip.h", _lib.SIGNATURES)
    published = sorted(h[len("include/"):] for h in LEDGER if h.startswith("include/"))
    assert published == sorted(os.listdir(os.path.join(ROOT, "include"))) and len(published) == 11 and "vnet_bbox.h" not in published


def test_no_name_is_declared_or_bound_twice():
    declared = [(h, set(guard.header_functions(os.path.join(ROOT, h)))) for h, _ in _lib.HEADERS]
    bound = [(h, set(t)) for h, t in _lib.HEADERS]
    for sets in (declared, bound):
        for i, (a, na) in enumerate(sets):
            for b, nb in sets[i + 1:]:
                assert not na & nb, (a, b, sorted(na & nb))
    assert len(_lib.all_signatures()) == sum(len(t) for _, t in _lib.HEADERS) == sum(len(row[1]) for row in LEDGER.values())
    twice = _lib.HEADERS + (("again.h", {"vnet_cc_roots": _lib.SIGNATURES_COMPONENTS["vnet_cc_roots"]}),)
    saved, _lib.HEADERS = _lib.HEADERS, twice
    try:
        with pytest.raises(ValueError, match="vnet_cc_roots"):
            _lib.all_signatures()
    finally:
        _lib.HEADERS = saved


def test_memoised_queries_are_the_set_memoised_before_the_rule():
    """By the rule and in the bound library (a memoised query is a Python closure, every other entry point a ctypes function)."""
    sigs = _lib.all_signatures()
    assert not MEMOISED & MEMOISED_SINCE
    assert set(n for n in sigs if _lib.memoised(n)) == MEMOISED | MEMOISED_SINCE
    L = _lib.lib()
    assert set(n for n in sigs if not isinstance(getattr(L, n), ctypes._CFuncPtr)) == MEMOISED | MEMOISED_SINCE
    assert not any(n.endswith("_ok") for n in (MEMOISED | MEMOISED_SINCE) - {"vnet_bn_head_ok"})


def test_isa_script_compiles_every_unit_of_the_makefile():
    srcs = re.search(r"^SRCS = (.*)$", _read("vnet_tensorflow_amd", "csrc", "Makefile"), re.M).group(1).split()
    loops = " ".join(re.findall(r"^for f in ([^;]*);", _read("profiles", "check_isa.sh"), re.M)).split()
    assert len(srcs) == 18 and sorted(s[:-len(".hip")] for s in srcs) == sorted(loops)
