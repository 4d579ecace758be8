"""Convolution routing (ops.route) on the host, no GPU: for every convolution of the three bench networks and each of their modes
the record -- family, launch tag, workspace bytes, epilogue statistics rows, flops and bytes -- matches a table recorded from the
launches of one eager training step per network and mode (tags and workspace queries in launch order, and the `_vnet_stats`
rows of every convolution output, before routing moved into one function).  And the side-stream guard of a filter gradient
reads the same tag the launch carries.

Batch-norm routing (ops.bn_route) likewise: for every batch-norm of those networks and modes, and with cross-replica statistics on,
the record matches a table recorded from the `vnet_bn_*` entries each batch-norm op launched in one eager step (and the all-reduces
it made) before the choice moved into one function."""
import pytest

pytest.importorskip("torch")

from vnet_tensorflow_amd import ops  # noqa: E402

# (network, mode) -> (op, tag, family, workspace bytes, statistics rows, flops, bytes) of every distinct launch of a step
EXPECTED = {
    ('C3', 'fp32'): [
        ('input-fwd', 'input-direct 128^3x1 1->16', 'input-direct', 0, 2048, 8388608000, 142606336),
        ('fwd', 'conv k2 s2 64^3x1 16->32', 'conv2-direct', 0, 2048, 2147483648, 167788544),
        ('fwd', 'conv k5 s1 64^3x1 32->32', 'conv', 0, 1024, 67108864000, 67620992),
        ('fwd', 'conv k2 s2 32^3x1 32->64', 'conv2-direct', 0, 256, 1073741824, 42008576),
        ('fwd', 'conv k5 s1 32^3x1 64->64', 'conv', 0, 128, 33554432000, 18825472),
        ('fwd', 'conv k2 s2 16^3x1 64->128', 'conv', 0, 64, 536870912, 10748416),
        ('fwd', 'conv k5 s1 16^3x1 128->128', 'conv', 16777216, 2048, 16777216000, 12386816),
        ('fwd', 'conv k2 s2 8^3x1 128->256', 'conv', 4194304, 512, 268435456, 3671040),
        ('fwd', 'conv k5 s1 8^3x1 256->256', 'conv', 8388608, 512, 8388608000, 33817600),
        ('fwd', 'conv k2 s2 up 16^3x1 256->128', 'conv', 0, 0, 268435456, 3670528),
        ('fwd', 'conv k5 s1 16^3x1 256->128', 'conv', 33554432, 2048, 33554432000, 22675968),
        ('fwd', 'conv k2 s2 up 32^3x1 128->64', 'conv', 0, 0, 536870912, 10748160),
        ('fwd', 'conv k5 s1 32^3x1 128->64', 'conv', 0, 128, 67108864000, 29262080),
        ('fwd', 'conv k2 s2 up 64^3x1 64->32', 'conv2-direct', 0, 0, 1073741824, 42008576),
        ('fwd', 'conv k5 s1 64^3x1 64->32', 'conv', 0, 1024, 134217728000, 101687424),
        ('fwd', 'conv k2 s2 up 128^3x1 32->16', 'conv2-direct', 0, 0, 2147483648, 167788544),
        ('fwd', 'conv k5 s1 128^3x1 32->16', 'conv', 0, 8192, 268435456000, 402909248),
        ('wgrad', 'wgrad k5 s1 128^3x1 32->16', 'wgrad', 32768000, 0, 268435456000, 402909184),
        ('bwd', 'conv k5 s1 128^3x1 16->32', 'conv', 0, 0, 268435456000, 402909312),
        ('wgrad', 'wgrad k2 s2 64^3x1 16->32', 'wgrad', 4194304, 0, 2147483648, 167788544),
        ('bwd', 'conv k2 s2 64^3x1 16->32', 'conv2-direct', 0, 0, 2147483648, 167788544),
        ('wgrad', 'wgrad k5 s1 64^3x1 32->32', 'wgrad', 32768000, 0, 67108864000, 67620864),
        ('bwd', 'conv k5 s1 64^3x1 32->32', 'conv', 0, 0, 67108864000, 67620992),
        ('wgrad', 'wgrad k5 s1 64^3x1 64->32', 'wgrad', 32768000, 0, 134217728000, 101687296),
        ('bwd', 'conv k5 s1 64^3x1 32->64', 'conv', 0, 0, 134217728000, 101687552),
        ('wgrad', 'wgrad k2 s2 32^3x1 32->64', 'wgrad', 8388608, 0, 1073741824, 42008576),
        ('bwd', 'conv k2 s2 32^3x1 32->64', 'conv2-direct', 0, 0, 1073741824, 42008576),
        ('wgrad', 'wgrad k5 s1 32^3x1 64->64', 'wgrad', 32768000, 0, 33554432000, 18825216),
        ('bwd', 'conv k5 s1 32^3x1 64->64', 'conv', 0, 0, 33554432000, 18825472),
        ('wgrad', 'wgrad k5 s1 32^3x1 128->64', 'wgrad', 32768000, 0, 67108864000, 29261824),
        ('bwd', 'conv k5 s1 32^3x1 64->128', 'conv', 0, 0, 67108864000, 29262336),
        ('wgrad', 'wgrad k2 s2 16^3x1 64->128', 'wgrad', 8388608, 0, 536870912, 10747904),
        ('bwd', 'conv k2 s2 16^3x1 64->128', 'conv', 0, 0, 536870912, 10748416),
        ('wgrad', 'wgrad k5 s1 16^3x1 128->128', 'wgrad', 32768000, 0, 16777216000, 12386304),
        ('bwd', 'conv k5 s1 16^3x1 128->128', 'conv', 16777216, 0, 16777216000, 12386816),
        ('wgrad', 'wgrad k5 s1 16^3x1 256->128', 'wgrad', 32768000, 0, 33554432000, 22675456),
        ('bwd', 'conv k5 s1 16^3x1 128->256', 'conv', 0, 0, 33554432000, 22676480),
        ('wgrad', 'wgrad k2 s2 8^3x1 128->256', 'wgrad', 4194304, 0, 268435456, 3670016),
        ('bwd', 'conv k2 s2 8^3x1 128->256', 'conv', 4194304, 0, 268435456, 3671040),
        ('wgrad', 'wgrad k5 s1 8^3x1 256->256', 'wgrad', 32768000, 0, 8388608000, 33816576),
        ('bwd', 'conv k5 s1 8^3x1 256->256', 'conv', 8388608, 0, 8388608000, 33817600),
        ('bwd', 'conv k2 s2 up 16^3x1 256->128', 'conv', 0, 0, 268435456, 3670528),
        ('bwd', 'conv k2 s2 up 32^3x1 128->64', 'conv', 0, 0, 536870912, 10748160),
        ('bwd', 'conv k2 s2 up 64^3x1 64->32', 'conv2-direct', 0, 0, 1073741824, 42008576),
        ('bwd', 'conv k2 s2 up 128^3x1 32->16', 'conv2-direct', 0, 0, 2147483648, 167788544),
        ('input-wgrad', 'input-wgrad-direct 128^3x1 1->16', 'input-wgrad-direct', 13107200, 0, 8388608000, 142606336),
    ],
    ('C3', 'fp32_split3'): [
        ('input-fwd', 'input-direct 128^3x1 1->16', 'input-direct', 0, 2048, 8388608000, 142606336),
        ('fwd', 'conv k2 s2 64^3x1 16->32', 'conv2-direct', 0, 2048, 2147483648, 167788544),
        ('fwd', 'conv-x3 k5 s1 64^3x1 32->32', 'conv-x3', 0, 1024, 67108864000, 67620992),
        ('fwd', 'conv k2 s2 32^3x1 32->64', 'conv2-direct', 0, 256, 1073741824, 42008576),
        ('fwd', 'conv-x3 k5 s1 32^3x1 64->64', 'conv-x3', 0, 128, 33554432000, 18825472),
        ('fwd', 'conv k2 s2 16^3x1 64->128', 'conv', 0, 64, 536870912, 10748416),
        ('fwd', 'conv-x3 k5 s1 16^3x1 128->128', 'conv-x3', 4194304, 2048, 16777216000, 12386816),
        ('fwd', 'conv k2 s2 8^3x1 128->256', 'conv', 4194304, 512, 268435456, 3671040),
        ('fwd', 'conv-x3 k5 s1 8^3x1 256->256', 'conv-x3', 4194304, 512, 8388608000, 33817600),
        ('fwd', 'conv k2 s2 up 16^3x1 256->128', 'conv', 0, 0, 268435456, 3670528),
        ('fwd', 'conv-x3 k5 s1 16^3x1 256->128', 'conv-x3', 4194304, 2048, 33554432000, 22675968),
        ('fwd', 'conv k2 s2 up 32^3x1 128->64', 'conv', 0, 0, 536870912, 10748160),
        ('fwd', 'conv-x3 k5 s1 32^3x1 128->64', 'conv-x3', 0, 128, 67108864000, 29262080),
        ('fwd', 'conv k2 s2 up 64^3x1 64->32', 'conv2-direct', 0, 0, 1073741824, 42008576),
        ('fwd', 'conv-x3 k5 s1 64^3x1 64->32', 'conv-x3', 0, 1024, 134217728000, 101687424),
        ('fwd', 'conv k2 s2 up 128^3x1 32->16', 'conv2-direct', 0, 0, 2147483648, 167788544),
        ('fwd', 'conv-x3 k5 s1 128^3x1 32->16', 'conv-x3', 0, 8192, 268435456000, 402909248),
        ('wgrad', 'wgrad-x3 k5 s1 128^3x1 32->16', 'wgrad-x3', 32768000, 0, 268435456000, 402909184),
        ('bwd', 'conv-x3 k5 s1 128^3x1 16->32', 'conv-x3', 0, 0, 268435456000, 402909312),
        ('wgrad', 'wgrad k2 s2 64^3x1 16->32', 'wgrad', 4194304, 0, 2147483648, 167788544),
        ('bwd', 'conv k2 s2 64^3x1 16->32', 'conv2-direct', 0, 0, 2147483648, 167788544),
        ('wgrad', 'wgrad-x3 k5 s1 64^3x1 32->32', 'wgrad-x3', 32768000, 0, 67108864000, 67620864),
        ('bwd', 'conv-x3 k5 s1 64^3x1 32->32', 'conv-x3', 0, 0, 67108864000, 67620992),
        ('wgrad', 'wgrad-x3 k5 s1 64^3x1 64->32', 'wgrad-x3', 32768000, 0, 134217728000, 101687296),
        ('bwd', 'conv-x3 k5 s1 64^3x1 32->64', 'conv-x3', 0, 0, 134217728000, 101687552),
        ('wgrad', 'wgrad k2 s2 32^3x1 32->64', 'wgrad', 8388608, 0, 1073741824, 42008576),
        ('bwd', 'conv k2 s2 32^3x1 32->64', 'conv2-direct', 0, 0, 1073741824, 42008576),
        ('wgrad', 'wgrad-x3 k5 s1 32^3x1 64->64', 'wgrad-x3', 32768000, 0, 33554432000, 18825216),
        ('bwd', 'conv-x3 k5 s1 32^3x1 64->64', 'conv-x3', 0, 0, 33554432000, 18825472),
        ('wgrad', 'wgrad-x3 k5 s1 32^3x1 128->64', 'wgrad-x3', 32768000, 0, 67108864000, 29261824),
        ('bwd', 'conv-x3 k5 s1 32^3x1 64->128', 'conv-x3', 0, 0, 67108864000, 29262336),
        ('wgrad', 'wgrad k2 s2 16^3x1 64->128', 'wgrad', 8388608, 0, 536870912, 10747904),
        ('bwd', 'conv k2 s2 16^3x1 64->128', 'conv', 0, 0, 536870912, 10748416),
        ('wgrad', 'wgrad-x3 k5 s1 16^3x1 128->128', 'wgrad-x3', 32768000, 0, 16777216000, 12386304),
        ('bwd', 'conv-x3 k5 s1 16^3x1 128->128', 'conv-x3', 4194304, 0, 16777216000, 12386816),
        ('wgrad', 'wgrad-x3 k5 s1 16^3x1 256->128', 'wgrad-x3', 32768000, 0, 33554432000, 22675456),
        ('bwd', 'conv-x3 k5 s1 16^3x1 128->256', 'conv-x3', 0, 0, 33554432000, 22676480),
        ('wgrad', 'wgrad k2 s2 8^3x1 128->256', 'wgrad', 4194304, 0, 268435456, 3670016),
        ('bwd', 'conv k2 s2 8^3x1 128->256', 'conv', 4194304, 0, 268435456, 3671040),
        ('wgrad', 'wgrad-x3 k5 s1 8^3x1 256->256', 'wgrad-x3', 32768000, 0, 8388608000, 33816576),
        ('bwd', 'conv-x3 k5 s1 8^3x1 256->256', 'conv-x3', 4194304, 0, 8388608000, 33817600),
        ('bwd', 'conv k2 s2 up 16^3x1 256->128', 'conv', 0, 0, 268435456, 3670528),
        ('bwd', 'conv k2 s2 up 32^3x1 128->64', 'conv', 0, 0, 536870912, 10748160),
        ('bwd', 'conv k2 s2 up 64^3x1 64->32', 'conv2-direct', 0, 0, 1073741824, 42008576),
        ('bwd', 'conv k2 s2 up 128^3x1 32->16', 'conv2-direct', 0, 0, 2147483648, 167788544),
        ('input-wgrad', 'input-wgrad-direct 128^3x1 1->16', 'input-wgrad-direct', 13107200, 0, 8388608000, 142606336),
    ],
    ('C2', 'fp32'): [
        ('input-fwd', 'input-direct 64^3x2 1->16', 'input-direct', 0, 512, 2097152000, 35651584),
        ('fwd', 'conv k2 s2 32^3x2 16->32', 'conv2-direct', 0, 512, 536870912, 41959424),
        ('fwd', 'conv k5 s1 32^3x2 32->32', 'conv', 0, 256, 16777216000, 17289344),
        ('fwd', 'conv k2 s2 16^3x2 32->64', 'conv2-direct', 0, 64, 268435456, 10551296),
        ('fwd', 'conv k5 s1 16^3x2 64->64', 'conv', 8388608, 2048, 8388608000, 6242560),
        ('fwd', 'conv k2 s2 8^3x2 64->128', 'conv', 2097152, 512, 134217728, 2884096),
        ('fwd', 'conv k5 s1 8^3x2 128->128', 'conv', 4194304, 512, 4194304000, 9241088),
        ('fwd', 'conv k2 s2 4^3x2 128->256', 'conv', 1048576, 128, 67108864, 1704960),
        ('fwd', 'conv k5 s1 4^3x2 256->256', 'conv', 2097152, 128, 2097152000, 33031168),
        ('fwd', 'conv k2 s2 up 8^3x2 256->128', 'conv', 0, 0, 67108864, 1704448),
        ('fwd', 'conv k5 s1 8^3x2 256->128', 'conv', 8388608, 512, 8388608000, 17957376),
        ('fwd', 'conv k2 s2 up 16^3x2 128->64', 'conv', 0, 0, 134217728, 2883840),
        ('fwd', 'conv k5 s1 16^3x2 128->64', 'conv', 16777216, 2048, 16777216000, 10387712),
        ('fwd', 'conv k2 s2 up 32^3x2 64->32', 'conv2-direct', 0, 0, 268435456, 10551296),
        ('fwd', 'conv k5 s1 32^3x2 64->32', 'conv', 0, 256, 33554432000, 26189952),
        ('fwd', 'conv k2 s2 up 64^3x2 32->16', 'conv2-direct', 0, 0, 536870912, 41959424),
        ('fwd', 'conv k5 s1 64^3x2 32->16', 'conv', 0, 2048, 67108864000, 100919360),
        ('wgrad', 'wgrad k5 s1 64^3x2 32->16', 'wgrad', 32768000, 0, 67108864000, 100919296),
        ('bwd', 'conv k5 s1 64^3x2 16->32', 'conv', 0, 0, 67108864000, 100919424),
        ('wgrad', 'wgrad k2 s2 32^3x2 16->32', 'wgrad', 4194304, 0, 536870912, 41959424),
        ('bwd', 'conv k2 s2 32^3x2 16->32', 'conv2-direct', 0, 0, 536870912, 41959424),
        ('wgrad', 'wgrad k5 s1 32^3x2 32->32', 'wgrad', 32768000, 0, 16777216000, 17289216),
        ('bwd', 'conv k5 s1 32^3x2 32->32', 'conv', 0, 0, 16777216000, 17289344),
        ('wgrad', 'wgrad k5 s1 32^3x2 64->32', 'wgrad', 32768000, 0, 33554432000, 26189824),
        ('bwd', 'conv k5 s1 32^3x2 32->64', 'conv', 0, 0, 33554432000, 26190080),
        ('wgrad', 'wgrad k2 s2 16^3x2 32->64', 'wgrad', 4194304, 0, 268435456, 10551296),
        ('bwd', 'conv k2 s2 16^3x2 32->64', 'conv2-direct', 0, 0, 268435456, 10551296),
        ('wgrad', 'wgrad k5 s1 16^3x2 64->64', 'wgrad', 32768000, 0, 8388608000, 6242304),
        ('bwd', 'conv k5 s1 16^3x2 64->64', 'conv', 8388608, 0, 8388608000, 6242560),
        ('wgrad', 'wgrad k5 s1 16^3x2 128->64', 'wgrad', 32768000, 0, 16777216000, 10387456),
        ('bwd', 'conv k5 s1 16^3x2 64->128', 'conv', 0, 0, 16777216000, 10387968),
        ('wgrad', 'wgrad k2 s2 8^3x2 64->128', 'wgrad', 2097152, 0, 134217728, 2883584),
        ('bwd', 'conv k2 s2 8^3x2 64->128', 'conv', 2097152, 0, 134217728, 2884096),
        ('wgrad', 'wgrad k5 s1 8^3x2 128->128', 'wgrad', 32768000, 0, 4194304000, 9240576),
        ('bwd', 'conv k5 s1 8^3x2 128->128', 'conv', 4194304, 0, 4194304000, 9241088),
        ('wgrad', 'wgrad k5 s1 8^3x2 256->128', 'wgrad', 32768000, 0, 8388608000, 17956864),
        ('bwd', 'conv k5 s1 8^3x2 128->256', 'conv', 8388608, 0, 8388608000, 17957888),
        ('wgrad', 'wgrad k2 s2 4^3x2 128->256', 'wgrad', 4194304, 0, 67108864, 1703936),
        ('bwd', 'conv k2 s2 4^3x2 128->256', 'conv', 1048576, 0, 67108864, 1704960),
        ('wgrad', 'wgrad k5 s1 4^3x2 256->256', 'wgrad', 32768000, 0, 2097152000, 33030144),
        ('bwd', 'conv k5 s1 4^3x2 256->256', 'conv', 2097152, 0, 2097152000, 33031168),
        ('bwd', 'conv k2 s2 up 8^3x2 256->128', 'conv', 0, 0, 67108864, 1704448),
        ('bwd', 'conv k2 s2 up 16^3x2 128->64', 'conv', 0, 0, 134217728, 2883840),
        ('bwd', 'conv k2 s2 up 32^3x2 64->32', 'conv2-direct', 0, 0, 268435456, 10551296),
        ('bwd', 'conv k2 s2 up 64^3x2 32->16', 'conv2-direct', 0, 0, 536870912, 41959424),
        ('input-wgrad', 'input-wgrad-direct 64^3x2 1->16', 'input-wgrad-direct', 13107200, 0, 2097152000, 35651584),
    ],
    ('C2', 'fp32_split3'): [
        ('input-fwd', 'input-direct 64^3x2 1->16', 'input-direct', 0, 512, 2097152000, 35651584),
        ('fwd', 'conv k2 s2 32^3x2 16->32', 'conv2-direct', 0, 512, 536870912, 41959424),
        ('fwd', 'conv-x3 k5 s1 32^3x2 32->32', 'conv-x3', 0, 256, 16777216000, 17289344),
        ('fwd', 'conv k2 s2 16^3x2 32->64', 'conv2-direct', 0, 64, 268435456, 10551296),
        ('fwd', 'conv-x3 k5 s1 16^3x2 64->64', 'conv-x3', 4194304, 2048, 8388608000, 6242560),
        ('fwd', 'conv k2 s2 8^3x2 64->128', 'conv', 2097152, 512, 134217728, 2884096),
        ('fwd', 'conv k5 s1 8^3x2 128->128', 'conv', 4194304, 512, 4194304000, 9241088),
        ('fwd', 'conv k2 s2 4^3x2 128->256', 'conv', 1048576, 128, 67108864, 1704960),
        ('fwd', 'conv k5 s1 4^3x2 256->256', 'conv', 2097152, 128, 2097152000, 33031168),
        ('fwd', 'conv k2 s2 up 8^3x2 256->128', 'conv', 0, 0, 67108864, 1704448),
        ('fwd', 'conv-x3 k5 s1 8^3x2 256->128', 'conv-x3', 4194304, 512, 8388608000, 17957376),
        ('fwd', 'conv k2 s2 up 16^3x2 128->64', 'conv', 0, 0, 134217728, 2883840),
        ('fwd', 'conv-x3 k5 s1 16^3x2 128->64', 'conv-x3', 4194304, 2048, 16777216000, 10387712),
        ('fwd', 'conv k2 s2 up 32^3x2 64->32', 'conv2-direct', 0, 0, 268435456, 10551296),
        ('fwd', 'conv-x3 k5 s1 32^3x2 64->32', 'conv-x3', 0, 256, 33554432000, 26189952),
        ('fwd', 'conv k2 s2 up 64^3x2 32->16', 'conv2-direct', 0, 0, 536870912, 41959424),
        ('fwd', 'conv-x3 k5 s1 64^3x2 32->16', 'conv-x3', 0, 2048, 67108864000, 100919360),
        ('wgrad', 'wgrad-x3 k5 s1 64^3x2 32->16', 'wgrad-x3', 32768000, 0, 67108864000, 100919296),
        ('bwd', 'conv-x3 k5 s1 64^3x2 16->32', 'conv-x3', 0, 0, 67108864000, 100919424),
        ('wgrad', 'wgrad k2 s2 32^3x2 16->32', 'wgrad', 4194304, 0, 536870912, 41959424),
        ('bwd', 'conv k2 s2 32^3x2 16->32', 'conv2-direct', 0, 0, 536870912, 41959424),
        ('wgrad', 'wgrad-x3 k5 s1 32^3x2 32->32', 'wgrad-x3', 32768000, 0, 16777216000, 17289216),
        ('bwd', 'conv-x3 k5 s1 32^3x2 32->32', 'conv-x3', 0, 0, 16777216000, 17289344),
        ('wgrad', 'wgrad-x3 k5 s1 32^3x2 64->32', 'wgrad-x3', 32768000, 0, 33554432000, 26189824),
        ('bwd', 'conv-x3 k5 s1 32^3x2 32->64', 'conv-x3', 0, 0, 33554432000, 26190080),
        ('wgrad', 'wgrad k2 s2 16^3x2 32->64', 'wgrad', 4194304, 0, 268435456, 10551296),
        ('bwd', 'conv k2 s2 16^3x2 32->64', 'conv2-direct', 0, 0, 268435456, 10551296),
        ('wgrad', 'wgrad k5 s1 16^3x2 64->64', 'wgrad', 32768000, 0, 8388608000, 6242304),
        ('bwd', 'conv-x3 k5 s1 16^3x2 64->64', 'conv-x3', 4194304, 0, 8388608000, 6242560),
        ('wgrad', 'wgrad-x3 k5 s1 16^3x2 128->64', 'wgrad-x3', 32768000, 0, 16777216000, 10387456),
        ('bwd', 'conv-x3 k5 s1 16^3x2 64->128', 'conv-x3', 0, 0, 16777216000, 10387968),
        ('wgrad', 'wgrad k2 s2 8^3x2 64->128', 'wgrad', 2097152, 0, 134217728, 2883584),
        ('bwd', 'conv k2 s2 8^3x2 64->128', 'conv', 2097152, 0, 134217728, 2884096),
        ('wgrad', 'wgrad k5 s1 8^3x2 128->128', 'wgrad', 32768000, 0, 4194304000, 9240576),
        ('bwd', 'conv k5 s1 8^3x2 128->128', 'conv', 4194304, 0, 4194304000, 9241088),
        ('wgrad', 'wgrad-x3 k5 s1 8^3x2 256->128', 'wgrad-x3', 32768000, 0, 8388608000, 17956864),
        ('bwd', 'conv-x3 k5 s1 8^3x2 128->256', 'conv-x3', 4194304, 0, 8388608000, 17957888),
        ('wgrad', 'wgrad k2 s2 4^3x2 128->256', 'wgrad', 4194304, 0, 67108864, 1703936),
        ('bwd', 'conv k2 s2 4^3x2 128->256', 'conv', 1048576, 0, 67108864, 1704960),
        ('wgrad', 'wgrad k5 s1 4^3x2 256->256', 'wgrad', 32768000, 0, 2097152000, 33030144),
        ('bwd', 'conv k5 s1 4^3x2 256->256', 'conv', 2097152, 0, 2097152000, 33031168),
        ('bwd', 'conv k2 s2 up 8^3x2 256->128', 'conv', 0, 0, 67108864, 1704448),
        ('bwd', 'conv k2 s2 up 16^3x2 128->64', 'conv', 0, 0, 134217728, 2883840),
        ('bwd', 'conv k2 s2 up 32^3x2 64->32', 'conv2-direct', 0, 0, 268435456, 10551296),
        ('bwd', 'conv k2 s2 up 64^3x2 32->16', 'conv2-direct', 0, 0, 536870912, 41959424),
        ('input-wgrad', 'input-wgrad-direct 64^3x2 1->16', 'input-wgrad-direct', 13107200, 0, 2097152000, 35651584),
    ],
    ('C5', 'bf16'): [
        ('fwd', 'conv-bf16 k5 s1 128^3x1 8->16', 'conv-bf16-padded', 0, 4096, 67108864000, 100695296),
        ('fwd', 'conv-bf16 k5 s1 128^3x1 16->16', 'conv-bf16', 0, 4096, 134217728000, 134281728),
        ('fwd', 'conv-b16 k2 s2 64^3x1 16->32', 'conv2-direct', 0, 2048, 2147483648, 83902464),
        ('fwd', 'conv-bf16 k5 s1 64^3x1 32->32', 'conv-bf16', 0, 256, 67108864000, 33810432),
        ('fwd', 'conv-b16 k2 s2 32^3x1 32->64', 'conv2-direct', 0, 256, 1073741824, 21037056),
        ('fwd', 'conv-bf16 k5 s1 32^3x1 64->64', 'conv-bf16', 0, 128, 33554432000, 9412608),
        ('fwd', 'conv-b16 k2 s2 16^3x1 64->128', 'conv2-b16', 0, 64, 536870912, 5505024),
        ('fwd', 'conv-bf16 k5 s1 16^3x1 128->128', 'conv-bf16', 16777216, 2048, 16777216000, 6193152),
        ('fwd', 'conv-b16 k2 s2 8^3x1 128->256', 'conv2-b16', 4194304, 512, 268435456, 2359296),
        ('fwd', 'conv-bf16 k5 s1 8^3x1 256->256', 'conv-bf16', 8388608, 512, 8388608000, 16908288),
        ('fwd', 'conv-b16 k2 s2 up 16^3x1 256->128', 'conv2-b16', 0, 0, 268435456, 2359296),
        ('fwd', 'conv-bf16 k5 s1 16^3x1 256->128', 'conv-bf16', 16777216, 2048, 33554432000, 11337728),
        ('fwd', 'conv-b16 k2 s2 up 32^3x1 128->64', 'conv2-b16', 0, 0, 536870912, 5505024),
        ('fwd', 'conv-bf16 k5 s1 32^3x1 128->64', 'conv-bf16', 0, 128, 67108864000, 14630912),
        ('fwd', 'conv-b16 k2 s2 up 64^3x1 64->32', 'conv2-direct', 0, 0, 1073741824, 21037056),
        ('fwd', 'conv-bf16 k5 s1 64^3x1 64->32', 'conv-bf16', 0, 256, 134217728000, 50843648),
        ('fwd', 'conv-b16 k2 s2 up 128^3x1 32->16', 'conv2-direct', 0, 0, 2147483648, 83902464),
        ('fwd', 'conv-bf16 k5 s1 128^3x1 32->16', 'conv-bf16', 0, 4096, 268435456000, 201454592),
        ('wgrad', 'wgrad-bf16 k5 s1 128^3x1 32->16', 'wgrad-bf16', 32768000, 0, 268435456000, 201582592),
        ('bwd', 'conv-bf16 k5 s1 128^3x1 16->32', 'conv-bf16', 0, 0, 268435456000, 201454592),
        ('wgrad', 'wgrad-b16 k2 s2 64^3x1 16->32', 'wgrad2-b16', 4194304, 0, 2147483648, 83902464),
        ('bwd', 'conv-b16 k2 s2 64^3x1 16->32', 'conv2-direct', 0, 0, 2147483648, 83902464),
        ('wgrad', 'wgrad-bf16 k5 s1 64^3x1 32->32', 'wgrad-bf16', 32768000, 0, 67108864000, 34066432),
        ('bwd', 'conv-bf16 k5 s1 64^3x1 32->32', 'conv-bf16', 0, 0, 67108864000, 33810432),
        ('wgrad', 'wgrad-bf16 k5 s1 64^3x1 64->32', 'wgrad-bf16', 32768000, 0, 134217728000, 51355648),
        ('bwd', 'conv-bf16 k5 s1 64^3x1 32->64', 'conv-bf16', 0, 0, 134217728000, 50843648),
        ('wgrad', 'wgrad-b16 k2 s2 32^3x1 32->64', 'wgrad2-b16', 8388608, 0, 1073741824, 21037056),
        ('bwd', 'conv-b16 k2 s2 32^3x1 32->64', 'conv2-direct', 0, 0, 1073741824, 21037056),
        ('wgrad', 'wgrad-bf16 k5 s1 32^3x1 64->64', 'wgrad-bf16', 32768000, 0, 33554432000, 10436608),
        ('bwd', 'conv-bf16 k5 s1 32^3x1 64->64', 'conv-bf16', 0, 0, 33554432000, 9412608),
        ('wgrad', 'wgrad-bf16 k5 s1 32^3x1 128->64', 'wgrad-bf16', 32768000, 0, 67108864000, 16678912),
        ('bwd', 'conv-bf16 k5 s1 32^3x1 64->128', 'conv-bf16', 0, 0, 67108864000, 14630912),
        ('wgrad', 'wgrad-b16 k2 s2 16^3x1 64->128', 'wgrad2-b16', 8388608, 0, 536870912, 5505024),
        ('bwd', 'conv-b16 k2 s2 16^3x1 64->128', 'conv2-b16', 0, 0, 536870912, 5505024),
        ('wgrad', 'wgrad-bf16 k5 s1 16^3x1 128->128', 'wgrad-bf16', 32768000, 0, 16777216000, 10289152),
        ('bwd', 'conv-bf16 k5 s1 16^3x1 128->128', 'conv-bf16', 16777216, 0, 16777216000, 6193152),
        ('wgrad', 'wgrad-bf16 k5 s1 16^3x1 256->128', 'wgrad-bf16', 32768000, 0, 33554432000, 19529728),
        ('bwd', 'conv-bf16 k5 s1 16^3x1 128->256', 'conv-bf16', 16777216, 0, 33554432000, 11337728),
        ('wgrad', 'wgrad-b16 k2 s2 8^3x1 128->256', 'wgrad2-b16', 4194304, 0, 268435456, 2359296),
        ('bwd', 'conv-b16 k2 s2 8^3x1 128->256', 'conv2-b16', 4194304, 0, 268435456, 2359296),
        ('wgrad', 'wgrad-bf16 k5 s1 8^3x1 256->256', 'wgrad-bf16', 32768000, 0, 8388608000, 33292288),
        ('bwd', 'conv-bf16 k5 s1 8^3x1 256->256', 'conv-bf16', 8388608, 0, 8388608000, 16908288),
        ('bwd', 'conv-b16 k2 s2 up 16^3x1 256->128', 'conv2-b16', 0, 0, 268435456, 2359296),
        ('bwd', 'conv-b16 k2 s2 up 32^3x1 128->64', 'conv2-b16', 0, 0, 536870912, 5505024),
        ('bwd', 'conv-b16 k2 s2 up 64^3x1 64->32', 'conv2-direct', 0, 0, 1073741824, 21037056),
        ('bwd', 'conv-b16 k2 s2 up 128^3x1 32->16', 'conv2-direct', 0, 0, 2147483648, 83902464),
        ('wgrad', 'wgrad-bf16 k5 s1 128^3x1 16->16', 'wgrad-bf16', 32768000, 0, 134217728000, 134345728),
        ('bwd', 'conv-bf16 k5 s1 128^3x1 16->16', 'conv-bf16', 0, 0, 134217728000, 134281728),
        ('wgrad', 'wgrad-bf16 k5 s1 128^3x1 8->16', 'wgrad-bf16', 32768000, 0, 67108864000, 100727296),
    ],
}

# network -> (patch, batch, input channels): bench.py's V-Net, 16 channels, 4 levels, (1, 2, 3, 3) convolutions, 3 at the bottom
NETWORKS = {"C3": (128, 1, 1), "C2": (64, 2, 1), "C5": (128, 1, 4)}
LEVEL_CONVS, BOTTOM_CONVS, CH = (1, 2, 3, 3), 3, 16


def vnet_convolutions(P, cin):
    """(ks, stride, up, C0, C1, O, din, dout, cin) of every convolution layer of the network, in forward order; the 1-channel
    input block as ("input", O, dims)."""
    out = []
    dims = lambda l: (P >> l,) * 3
    if cin == 1:
        out.append(("input", CH, dims(0)))                               # tile + batch-norm + level 0's convolution, fused
    else:
        out.append((5, 1, 0, -(-cin // 8) * 8, 0, CH, dims(0), dims(0), cin))   # the cast input, zero-padded to 8 channels
        out += [(5, 1, 0, CH, 0, CH, dims(0), dims(0), CH)] * LEVEL_CONVS[0]
    for l, n in list(enumerate(LEVEL_CONVS))[1:] + [(len(LEVEL_CONVS), BOTTOM_CONVS)]:
        c = CH << l
        out.append((2, 2, 0, c // 2, 0, c, dims(l - 1), dims(l), c // 2))      # down convolution
        out += [(5, 1, 0, c, 0, c, dims(l), dims(l), c)] * n
    for l in reversed(range(len(LEVEL_CONVS))):
        c = CH << l
        out.append((2, 2, 1, 2 * c, 0, c, dims(l + 1), dims(l), 2 * c))      # up convolution (filter [2,2,2,c,2c])
        out.append((5, 1, 0, c, c, c, dims(l), dims(l), 2 * c))              # on concat(up, skip)
        out += [(5, 1, 0, c, 0, c, dims(l), dims(l), c)] * (LEVEL_CONVS[l] - 1)
    return out


def routes(net, mode):
    P, B, cin = NETWORKS[net]
    bf16, split3 = mode == "bf16", mode == "fp32_split3"
    got = {}

    def add(op, r):
        ent = (r.family, r.ws, r.stats_rows, int(r.flops), int(r.nbytes))
        assert got.setdefault((op, r.tag), ent) == ent, (op, r.tag)
    for k, layer in enumerate(vnet_convolutions(P, cin)):
        if layer[0] == "input":
            _, O, d = layer
            for op in (ops.IN_FWD, ops.IN_WGRAD):
                add(op, ops.route(op, 5, 1, 0, False, False, 1, 0, O, B, d, d))
            continue
        ks, stride, up, C0, C1, O, din, dout, I = layer
        for op in (ops.FWD, ops.WGRAD) + ((ops.BWD,) if k > 0 else ()):         # (the first layer's input needs no gradient)
            add(op, ops.route(op, ks, stride, up, bf16, split3, C0, C1, O, B, din, dout, True, I))
    return got


@pytest.mark.parametrize("net,mode", sorted(EXPECTED))
def test_routes_of_the_bench_networks(net, mode):
    want = {(op, tag): (fam, ws, rows, fl, nb) for op, tag, fam, ws, rows, fl, nb in EXPECTED[(net, mode)]}
    assert routes(net, mode) == want


@pytest.mark.parametrize("mode,op,layer,tag", [
    ("fp32_split3", ops.WGRAD, (5, 1, 0, 16, 16, 16, (128,) * 3, (128,) * 3, 32), "wgrad-x3 k5 s1 128^3x1 32->16"),
    ("bf16", ops.WGRAD, (2, 2, 1, 32, 0, 16, (64,) * 3, (128,) * 3, 32), "wgrad-b16 k2 s2 64^3x1 16->32"),
    ("bf16", ops.WGRAD, (2, 2, 0, 16, 0, 32, (128,) * 3, (64,) * 3, 16), "wgrad-b16 k2 s2 64^3x1 16->32"),
    ("fp32", ops.WGRAD, (5, 1, 0, 32, 0, 32, (64,) * 3, (64,) * 3, 32), "wgrad k5 s1 64^3x1 32->32"),
])
def test_side_stream_guard_reads_the_launch_tag(monkeypatch, mode, op, layer, tag):
    """A filter gradient that is being timed stays on the main stream: the guard keys on the tag its launch carries."""
    ks, stride, up, C0, C1, O, din, dout, I = layer
    r = ops.route(op, ks, stride, up, mode == "bf16", mode == "fp32_split3", C0, C1, O, 1, din, dout, True, I)
    assert r.tag == tag
    side, sink = object(), object()
    monkeypatch.setattr(ops, "param_grad_stream", lambda dev: side)
    monkeypatch.setitem(ops._PROFILE, "on", True)
    monkeypatch.setitem(ops._PROFILE, "only", {tag})
    assert ops._side_stream("cuda", r, None, None, object(), sink) is None
    monkeypatch.setitem(ops._PROFILE, "only", {"conv k5 s1 64^3x1 32->32"})
    assert ops._side_stream("cuda", r, None, None, object(), sink) is side


# (network, mode, cross-replica statistics) -> (op, M, C, bcast, x16, r16, epilogue, stats, stats16, apply16, allreduce) of every
# distinct batch-norm of a step: its inputs -- op "act" (bn_act), "chain" (bn_chain), "stats" (a dead batch-norm's moving-average
# update); rows M, channels C, tiled 1-channel input, x / residual bf16 (r16 None: no residual), x carries matching epilogue sums --
# and the record its launches fix: statistics source and bf16-ness of the statistics and apply entries (a stats-only op launches no
# apply: its tensors' dtype), and whether the backward all-reduced its sums (a backward without a data gradient -- the tiled image --
# stops before that all-reduce: the statistics source decides).  Sync: two ranks over gloo.  C3 also in bf16 storage: the tiled
# image's batch-norm.
BN_EXPECTED = {
    ('C3', 'fp32', False): [
        ('act', 2097152, 16, True, False, None, False, 'stream', False, False, False),
        ('act', 2097152, 16, False, False, False, True, 'epilogue', False, False, False),
        ('act', 262144, 32, False, False, None, True, 'epilogue', False, False, False),
        ('act', 262144, 32, False, False, False, True, 'epilogue', False, False, False),
        ('act', 32768, 64, False, False, None, True, 'epilogue', False, False, False),
        ('act', 32768, 64, False, False, False, True, 'epilogue', False, False, False),
        ('act', 4096, 128, False, False, None, True, 'epilogue', False, False, False),
        ('act', 4096, 128, False, False, False, True, 'epilogue', False, False, False),
        ('act', 512, 256, False, False, None, True, 'epilogue', False, False, False),
        ('act', 512, 256, False, False, False, True, 'epilogue', False, False, False),
        ('act', 4096, 128, False, False, None, False, 'stream', False, False, False),
        ('stats', 4096, 128, False, False, None, True, 'epilogue', False, False, False),
        ('chain', 4096, 128, False, False, None, True, 'epilogue', False, False, False),
        ('act', 32768, 64, False, False, None, False, 'stream', False, False, False),
        ('stats', 32768, 64, False, False, None, True, 'epilogue', False, False, False),
        ('chain', 32768, 64, False, False, None, True, 'epilogue', False, False, False),
        ('act', 262144, 32, False, False, None, False, 'stream', False, False, False),
        ('chain', 262144, 32, False, False, None, True, 'epilogue', False, False, False),
        ('act', 2097152, 16, False, False, None, False, 'stream', False, False, False),
        ('chain', 2097152, 16, False, False, None, True, 'epilogue', False, False, False),
        ('act', 2097152, 2, False, False, None, False, 'stream', False, False, False),
    ],
    ('C3', 'fp32_split3', False): [
        ('act', 2097152, 16, True, False, None, False, 'stream', False, False, False),
        ('act', 2097152, 16, False, False, False, True, 'epilogue', False, False, False),
        ('act', 262144, 32, False, False, None, True, 'epilogue', False, False, False),
        ('act', 262144, 32, False, False, False, True, 'epilogue', False, False, False),
        ('act', 32768, 64, False, False, None, True, 'epilogue', False, False, False),
        ('act', 32768, 64, False, False, False, True, 'epilogue', False, False, False),
        ('act', 4096, 128, False, False, None, True, 'epilogue', False, False, False),
        ('act', 4096, 128, False, False, False, True, 'epilogue', False, False, False),
        ('act', 512, 256, False, False, None, True, 'epilogue', False, False, False),
        ('act', 512, 256, False, False, False, True, 'epilogue', False, False, False),
        ('act', 4096, 128, False, False, None, False, 'stream', False, False, False),
        ('stats', 4096, 128, False, False, None, True, 'epilogue', False, False, False),
        ('chain', 4096, 128, False, False, None, True, 'epilogue', False, False, False),
        ('act', 32768, 64, False, False, None, False, 'stream', False, False, False),
        ('stats', 32768, 64, False, False, None, True, 'epilogue', False, False, False),
        ('chain', 32768, 64, False, False, None, True, 'epilogue', False, False, False),
        ('act', 262144, 32, False, False, None, False, 'stream', False, False, False),
        ('chain', 262144, 32, False, False, None, True, 'epilogue', False, False, False),
        ('act', 2097152, 16, False, False, None, False, 'stream', False, False, False),
        ('chain', 2097152, 16, False, False, None, True, 'epilogue', False, False, False),
        ('act', 2097152, 2, False, False, None, False, 'stream', False, False, False),
    ],
    ('C2', 'fp32', False): [
        ('act', 524288, 16, True, False, None, False, 'stream', False, False, False),
        ('act', 524288, 16, False, False, False, True, 'epilogue', False, False, False),
        ('act', 65536, 32, False, False, None, True, 'epilogue', False, False, False),
        ('act', 65536, 32, False, False, False, True, 'epilogue', False, False, False),
        ('act', 8192, 64, False, False, None, True, 'epilogue', False, False, False),
        ('act', 8192, 64, False, False, False, True, 'epilogue', False, False, False),
        ('act', 1024, 128, False, False, None, True, 'epilogue', False, False, False),
        ('act', 1024, 128, False, False, False, True, 'epilogue', False, False, False),
        ('act', 128, 256, False, False, None, True, 'epilogue', False, False, False),
        ('act', 128, 256, False, False, False, True, 'epilogue', False, False, False),
        ('act', 1024, 128, False, False, None, False, 'stream', False, False, False),
        ('stats', 1024, 128, False, False, None, True, 'epilogue', False, False, False),
        ('chain', 1024, 128, False, False, None, True, 'epilogue', False, False, False),
        ('act', 8192, 64, False, False, None, False, 'stream', False, False, False),
        ('stats', 8192, 64, False, False, None, True, 'epilogue', False, False, False),
        ('chain', 8192, 64, False, False, None, True, 'epilogue', False, False, False),
        ('act', 65536, 32, False, False, None, False, 'stream', False, False, False),
        ('chain', 65536, 32, False, False, None, True, 'epilogue', False, False, False),
        ('act', 524288, 16, False, False, None, False, 'stream', False, False, False),
        ('chain', 524288, 16, False, False, None, True, 'epilogue', False, False, False),
        ('act', 524288, 2, False, False, None, False, 'stream', False, False, False),
    ],
    ('C2', 'fp32_split3', False): [
        ('act', 524288, 16, True, False, None, False, 'stream', False, False, False),
        ('act', 524288, 16, False, False, False, True, 'epilogue', False, False, False),
        ('act', 65536, 32, False, False, None, True, 'epilogue', False, False, False),
        ('act', 65536, 32, False, False, False, True, 'epilogue', False, False, False),
        ('act', 8192, 64, False, False, None, True, 'epilogue', False, False, False),
        ('act', 8192, 64, False, False, False, True, 'epilogue', False, False, False),
        ('act', 1024, 128, False, False, None, True, 'epilogue', False, False, False),
        ('act', 1024, 128, False, False, False, True, 'epilogue', False, False, False),
        ('act', 128, 256, False, False, None, True, 'epilogue', False, False, False),
        ('act', 128, 256, False, False, False, True, 'epilogue', False, False, False),
        ('act', 1024, 128, False, False, None, False, 'stream', False, False, False),
        ('stats', 1024, 128, False, False, None, True, 'epilogue', False, False, False),
        ('chain', 1024, 128, False, False, None, True, 'epilogue', False, False, False),
        ('act', 8192, 64, False, False, None, False, 'stream', False, False, False),
        ('stats', 8192, 64, False, False, None, True, 'epilogue', False, False, False),
        ('chain', 8192, 64, False, False, None, True, 'epilogue', False, False, False),
        ('act', 65536, 32, False, False, None, False, 'stream', False, False, False),
        ('chain', 65536, 32, False, False, None, True, 'epilogue', False, False, False),
        ('act', 524288, 16, False, False, None, False, 'stream', False, False, False),
        ('chain', 524288, 16, False, False, None, True, 'epilogue', False, False, False),
        ('act', 524288, 2, False, False, None, False, 'stream', False, False, False),
    ],
    ('C5', 'bf16', False): [
        ('act', 2097152, 16, False, True, None, True, 'epilogue', False, True, False),
        ('act', 2097152, 16, False, True, True, True, 'epilogue', False, True, False),
        ('act', 262144, 32, False, True, None, True, 'epilogue', False, True, False),
        ('act', 262144, 32, False, True, True, True, 'epilogue', False, True, False),
        ('act', 32768, 64, False, True, None, True, 'epilogue', False, True, False),
        ('act', 32768, 64, False, True, True, True, 'epilogue', False, True, False),
        ('act', 4096, 128, False, True, None, True, 'epilogue', False, True, False),
        ('act', 4096, 128, False, True, True, True, 'epilogue', False, True, False),
        ('act', 512, 256, False, True, None, True, 'small', True, True, False),
        ('act', 512, 256, False, True, True, True, 'small', True, True, False),
        ('act', 4096, 128, False, True, None, False, 'stream', True, True, False),
        ('stats', 4096, 128, False, True, None, True, 'epilogue', False, True, False),
        ('chain', 4096, 128, False, True, None, True, 'epilogue', False, True, False),
        ('act', 32768, 64, False, True, None, False, 'stream', True, True, False),
        ('stats', 32768, 64, False, True, None, True, 'epilogue', False, True, False),
        ('chain', 32768, 64, False, True, None, True, 'epilogue', False, True, False),
        ('act', 262144, 32, False, True, None, False, 'stream', True, True, False),
        ('chain', 262144, 32, False, True, None, True, 'epilogue', False, True, False),
        ('act', 2097152, 16, False, True, None, False, 'stream', True, True, False),
        ('chain', 2097152, 16, False, True, None, True, 'epilogue', False, True, False),
        ('act', 2097152, 5, False, False, None, False, 'stream', False, False, False),
    ],
    ('C3', 'bf16', False): [
        ('act', 2097152, 16, True, False, None, False, 'stream', False, True, False),
        ('act', 2097152, 16, False, True, True, True, 'epilogue', False, True, False),
        ('act', 262144, 32, False, True, None, True, 'epilogue', False, True, False),
        ('act', 262144, 32, False, True, True, True, 'epilogue', False, True, False),
        ('act', 32768, 64, False, True, None, True, 'epilogue', False, True, False),
        ('act', 32768, 64, False, True, True, True, 'epilogue', False, True, False),
        ('act', 4096, 128, False, True, None, True, 'epilogue', False, True, False),
        ('act', 4096, 128, False, True, True, True, 'epilogue', False, True, False),
        ('act', 512, 256, False, True, None, True, 'small', True, True, False),
        ('act', 512, 256, False, True, True, True, 'small', True, True, False),
        ('act', 4096, 128, False, True, None, False, 'stream', True, True, False),
        ('stats', 4096, 128, False, True, None, True, 'epilogue', False, True, False),
        ('chain', 4096, 128, False, True, None, True, 'epilogue', False, True, False),
        ('act', 32768, 64, False, True, None, False, 'stream', True, True, False),
        ('stats', 32768, 64, False, True, None, True, 'epilogue', False, True, False),
        ('chain', 32768, 64, False, True, None, True, 'epilogue', False, True, False),
        ('act', 262144, 32, False, True, None, False, 'stream', True, True, False),
        ('chain', 262144, 32, False, True, None, True, 'epilogue', False, True, False),
        ('act', 2097152, 16, False, True, None, False, 'stream', True, True, False),
        ('chain', 2097152, 16, False, True, None, True, 'epilogue', False, True, False),
        ('act', 2097152, 2, False, False, None, False, 'stream', False, False, False),
    ],
    ('C2', 'fp32', True): [
        ('act', 524288, 16, True, False, None, False, 'moments', False, False, True),
        ('act', 524288, 16, False, False, False, False, 'moments', False, False, True),
        ('act', 65536, 32, False, False, None, False, 'moments', False, False, True),
        ('act', 65536, 32, False, False, False, False, 'moments', False, False, True),
        ('act', 8192, 64, False, False, None, False, 'moments', False, False, True),
        ('act', 8192, 64, False, False, False, False, 'moments', False, False, True),
        ('act', 1024, 128, False, False, None, False, 'moments', False, False, True),
        ('act', 1024, 128, False, False, False, False, 'moments', False, False, True),
        ('act', 128, 256, False, False, None, False, 'moments', False, False, True),
        ('act', 128, 256, False, False, False, False, 'moments', False, False, True),
        ('stats', 1024, 128, False, False, None, False, 'moments', False, False, False),
        ('chain', 1024, 128, False, False, None, False, 'moments', False, False, True),
        ('stats', 8192, 64, False, False, None, False, 'moments', False, False, False),
        ('chain', 8192, 64, False, False, None, False, 'moments', False, False, True),
        ('chain', 65536, 32, False, False, None, False, 'moments', False, False, True),
        ('act', 524288, 16, False, False, None, False, 'moments', False, False, True),
        ('chain', 524288, 16, False, False, None, False, 'moments', False, False, True),
        ('act', 524288, 2, False, False, None, False, 'moments', False, False, True),
    ],
    ('C5', 'bf16', True): [
        ('act', 2097152, 16, False, True, None, False, 'moments', True, True, True),
        ('act', 2097152, 16, False, True, True, False, 'moments', True, True, True),
        ('act', 262144, 32, False, True, None, False, 'moments', True, True, True),
        ('act', 262144, 32, False, True, True, False, 'moments', True, True, True),
        ('act', 32768, 64, False, True, None, False, 'moments', True, True, True),
        ('act', 32768, 64, False, True, True, False, 'moments', True, True, True),
        ('act', 4096, 128, False, True, None, False, 'moments', True, True, True),
        ('act', 4096, 128, False, True, True, False, 'moments', True, True, True),
        ('act', 512, 256, False, True, None, False, 'moments', True, True, True),
        ('act', 512, 256, False, True, True, False, 'moments', True, True, True),
        ('stats', 4096, 128, False, True, None, False, 'moments', True, True, False),
        ('chain', 4096, 128, False, True, None, False, 'moments', True, True, True),
        ('stats', 32768, 64, False, True, None, False, 'moments', True, True, False),
        ('chain', 32768, 64, False, True, None, False, 'moments', True, True, True),
        ('chain', 262144, 32, False, True, None, False, 'moments', True, True, True),
        ('chain', 2097152, 16, False, True, None, False, 'moments', True, True, True),
        ('act', 2097152, 5, False, False, None, False, 'moments', False, False, True),
    ],
    ('C3', 'bf16', True): [
        ('act', 2097152, 16, True, False, None, False, 'moments', False, True, True),
        ('act', 2097152, 16, False, True, True, False, 'moments', True, True, True),
        ('act', 262144, 32, False, True, None, False, 'moments', True, True, True),
        ('act', 262144, 32, False, True, True, False, 'moments', True, True, True),
        ('act', 32768, 64, False, True, None, False, 'moments', True, True, True),
        ('act', 32768, 64, False, True, True, False, 'moments', True, True, True),
        ('act', 4096, 128, False, True, None, False, 'moments', True, True, True),
        ('act', 4096, 128, False, True, True, False, 'moments', True, True, True),
        ('act', 512, 256, False, True, None, False, 'moments', True, True, True),
        ('act', 512, 256, False, True, True, False, 'moments', True, True, True),
        ('stats', 4096, 128, False, True, None, False, 'moments', True, True, False),
        ('chain', 4096, 128, False, True, None, False, 'moments', True, True, True),
        ('stats', 32768, 64, False, True, None, False, 'moments', True, True, False),
        ('chain', 32768, 64, False, True, None, False, 'moments', True, True, True),
        ('chain', 262144, 32, False, True, None, False, 'moments', True, True, True),
        ('act', 2097152, 16, False, True, None, False, 'moments', True, True, True),
        ('chain', 2097152, 16, False, True, None, False, 'moments', True, True, True),
        ('act', 2097152, 2, False, False, None, False, 'moments', False, False, True),
    ],
}


@pytest.mark.parametrize("net,mode,sync", sorted(BN_EXPECTED))
def test_bn_routes_of_the_bench_networks(net, mode, sync):
    for op, M, C, bcast, x16, r16, epilogue, *want in BN_EXPECTED[(net, mode, sync)]:
        rt = ops.bn_route(op, M, C, bcast, x16, r16, epilogue, store16=mode == "bf16", sync=sync)
        assert tuple(rt) == tuple(want), (op, M, C, bcast, x16, r16, epilogue)


@pytest.mark.parametrize("args,kw,want", [
    (("act", 512, 256), dict(x16=True, epilogue=True), ("small", True, True, False)),       # small before the epilogue sums
    (("act", 512, 256), dict(x16=True, r16=False), ("stream", True, True, False)),          # fp32 residual (the forward refuses it)
    (("chain", 512, 256), dict(x16=True), ("stream", True, True, False)),                   # chains and dead batch-norms: never small
    (("stats", 512, 256), dict(x16=True, epilogue=True), ("epilogue", False, True, False)),
    (("act", 4096, 128), dict(x16=True, epilogue=True, sync=True), ("moments", True, True, True)),
    (("act", 4096, 16, True), dict(epilogue=True), ("stream", False, False, False)),        # (a tiled image carries no epilogue sums)
    (("act", 4096, 16, True), dict(store16=True), ("stream", False, True, False)),          # tiled image, bf16 storage: fp32 statistics
    (("act", 4096, 5, True), dict(store16=True), ("stream", False, False, False)),           # ... bf16 apply only for C = 8 * 2^k
])
def test_bn_route_precedence(args, kw, want):
    kw = dict(dict(store16=False, sync=False), **kw)
    assert tuple(ops.bn_route(*args, **kw)) == want


def test_bn_route_small_lever(monkeypatch):
    monkeypatch.setitem(ops._SMALL_BN, "on", False)
    assert tuple(ops.bn_route("act", 512, 256, x16=True, epilogue=True, store16=True, sync=False)) == ("epilogue", False, True, False)
    monkeypatch.setitem(ops._SMALL_BN, "on", True)
    monkeypatch.setitem(ops._SMALL_BN, "rows", 256)
    assert tuple(ops.bn_route("act", 512, 256, x16=True, store16=True, sync=False)) == ("stream", True, True, False)
