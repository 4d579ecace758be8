"""Host test: no float atomics under csrc/.  Every call of a HIP C++ atomic function is listed below with the reason its result does
not depend on the order in which the waves arrive -- all of them act on integers.  A float accumulated with atomicAdd gives other
bits from launch to launch (tests/test_hip_determinism.py; bn_act_bwd_reduce_kernel<2>, colsum_generic_kernel and
head_bwd_generic_kernel did so before they got a fixed order), so a new call has to be argued for here before the suite is green."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vnet_tensorflow_amd", "csrc")
CALL = re.compile(r"\b(atomicAdd|atomicMin|atomicMax|atomicCAS|atomicOr|atomicExch|__hip_atomic_\w+)\(")

COUNT = "integer counter: a sum of integers is the same in every order"
EXTREME = "integer minimum / maximum: order-independent"
UNION = ("union-find on int parents: every order of the links and path compressions leaves the same sets, and the labels are taken "
         "from the roots (the smallest index of a set) afterwards")
ALLOWED = {
    "components.hip": [
        ("if ((threadIdx.x & 63) == 0 && k) atomicMax(key, k);", "64-bit integer key count << 32 | ~representative: " + EXTREME),
    ],
    "score.hip": [
        ("if (acc_n && lane == 0) atomicAdd(cnt + acc_v * 3 + col, acc_n);", COUNT),
        ("if (v >= 0 && !same) atomicAdd(cnt + v * 3 + col, 1u);", COUNT),
        ("if (na) atomicAdd(cnt + va * 3 + 1, na);", COUNT),
        ("if (nb) atomicAdd(cnt + vb * 3 + 2, nb);", COUNT),
        ("if (ni) atomicAdd(cnt + vi * 3 + 0, ni);", COUNT),
        ("if (c) atomicAdd(out + i, (u64)c);", COUNT),
    ],
    "morph.hip": [
        ("atomicAdd(reinterpret_cast<u64*>(out7), (u64)count);", COUNT),
        ("atomicMin(out7 + 1, (i64)lo_a); atomicMin(out7 + 2, (i64)lo_b); atomicMin(out7 + 3, (i64)lo_c);", EXTREME),
        ("atomicMax(out7 + 4, (i64)hi_a); atomicMax(out7 + 5, (i64)hi_b); atomicMax(out7 + 6, (i64)hi_c);", EXTREME),
    ],
    "input_block.hip": [
        ("if (l >= 0 && l < K && p >= 0 && p < K) atomicAdd(&cm[l * K + p], 1u);", "the confusion matrix: " + COUNT),
        ("atomicAdd(&hist[(labels[i] == cls ? 0 : T + 1) + lo], 1u);", "the AUC histogram: " + COUNT),
    ],
    "sample.hip": [
        ("if (cnt) atomicAdd(out, (u64)cnt);", COUNT),
        ("if (sum) atomicAdd(out + 1, (u64)sum);       // (two's complement: a negative sum adds up all the same)",
         "64-bit integer sum of labels: " + COUNT),
    ],
    "cc_union.h": [
        ("const int p = __hip_atomic_load(parent + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);", UNION),
        ("const int old = atomicMin(parent + a, b);    // agent-scope RMW: a, a root when read, now hangs under the smaller root b", UNION),
        ("const int p = __hip_atomic_load(parent + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);", UNION),
        ("const int p = __hip_atomic_load(parent + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);", UNION),
        ("if (r != p) __hip_atomic_store(parent + idx, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);", UNION),
        ("if (acc_n && lane == 0) atomicAdd(sizes + acc_root, acc_n);", "component sizes: " + COUNT),
        ("if (fg && !same) atomicAdd(sizes + r, 1);", "component sizes: " + COUNT),
        ("if (sizes && acc_n && lane == 0) atomicAdd(sizes + acc_root, acc_n);", "component sizes: " + COUNT),
    ],
    "cc_table.h": [
        ("for (int a = 0; a < 3; ++a) { atomicMin(row + 2 + a, lo[a]); atomicMax(row + 5 + a, hi[a]); }", "bounding boxes: " + EXTREME),
        ("for (int a = 0; a < 3; ++a) atomicAdd(reinterpret_cast<u64*>(s) + a, (u64)v[a]);", "64-bit integer coordinate sums: " + COUNT),
    ],
}


def atomic_calls():
    """[(file, stripped line)] of every line under csrc/ that calls one of the functions of CALL, in file and line order."""
    out = []
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h", ".cpp", ".hpp", ".cu", ".cuh")):
            with open(os.path.join(CSRC, name)) as f:
                out.extend((name, line.strip()) for line in f if CALL.search(line))
    return out


def test_every_atomic_call_is_a_listed_integer_atomic():
    want = sorted((name, line) for name, rows in ALLOWED.items() for line, why in rows)
    assert all(why.strip() for rows in ALLOWED.values() for _, why in rows)
    got = sorted(atomic_calls())
    new = [c for c in got if c not in want]
    gone = [c for c in want if c not in got]
    assert not new, "atomic calls that are not in ALLOWED (a float atomic makes a result depend on the launch): %s" % new
    assert not gone, "ALLOWED lists calls the sources no longer make: %s" % gone
    assert got == want                                                           # (also as multisets: a line that occurs twice)
    assert not any(name == "elementwise.hip" for name, _ in got)
