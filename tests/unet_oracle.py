"""fp64 restatement of the reference's U-Net (networks.py:4-150) on the tape ops of oracle/vnet_oracle.py, plus the one op that
file does not have: 2x2x2 stride-2 VALID max-pooling whose gradient goes to the FIRST maximum of a window in (dz, dy, dx) scan
order (which tied voxel TF 1.15 picks cannot be verified here, and cannot matter in this network).
Written from the reference's graph code as a description of the wiring; shares no code with vnet_tensorflow_amd/."""
import numpy as np

from oracle import vnet_oracle as O


def max_pool2_fwd(x):
    """tf.nn.max_pool3d(x, [1,2,2,2,1], [1,2,2,2,1], 'VALID') on [B,D,H,W,C]: the eight window members [8,B,D/2,H/2,W/2,C] in scan
    order and their maximum."""
    B, D, H, W, C = x.shape
    d, h, w = D // 2, H // 2, W // 2
    win = np.stack([x[:, a:2 * d:2, b:2 * h:2, c:2 * w:2, :] for a in (0, 1) for b in (0, 1) for c in (0, 1)])
    return win, win.max(axis=0)


def max_pool2(x):
    win, y = max_pool2_fwd(x.v)
    out = O.Var(y, (x,))

    def bw(g):
        first = np.argmax(win == y[None], axis=0)            # index of the first member equal to the maximum
        dx = np.zeros_like(x.v)                              # (the trailing plane / row / column of an odd axis stays 0)
        d, h, w = y.shape[1:4]
        k = 0
        for a in (0, 1):
            for b in (0, 1):
                for c in (0, 1):
                    dx[:, a:2 * d:2, b:2 * h:2, c:2 * w:2, :] = np.where(first == k, g, 0.0)
                    k += 1
        x._acc(dx)
    out._bw = bw
    return out


class UNetOracle(object):
    def __init__(self, num_output_channels, dropout_rate=0.0, num_channels=4, num_levels=4, num_convolutions=2,
                 bottom_convolutions=2, activation_fn="relu", store=None):
        self.K, self.C, self.levels = num_output_channels, num_channels, num_levels
        self.convs, self.bottom, self.act = int(num_convolutions), int(bottom_convolutions), activation_fn
        assert dropout_rate == 0.0, "the oracle runs without dropout (TF's RNG stream is not reproducible)"
        self.ps = store if store is not None else O.ParamStore()

    def block(self, x, out_c, n):                             # networks.py:41-61
        ps = self.ps
        for i in range(n):
            with ps.variable_scope('conv_%d' % (i + 1)):
                x = O.L_convolution(ps, x, [3, 3, 3, x.v.shape[-1], out_c])
                x = O.L_batch_norm(ps, x)
                x = O.L_activation(ps, x, self.act)
        return x

    def block2(self, x, f, n):                                # networks.py:63-99
        ps = self.ps
        c = x.v.shape[-1]
        x = O.concat_channels(x, f)
        x = O.L_batch_norm(ps, x)                             # one batch-norm over the 2C channels
        for i in range(n):
            with ps.variable_scope('conv_%d' % (i + 1)):
                x = O.L_convolution(ps, x, [3, 3, 3, x.v.shape[-1], c])
            x = O.L_batch_norm(ps, x)                         # outside the conv_i scope
            x = O.L_activation(ps, x, self.act)
        return x

    def GetNetwork(self, images):                             # networks.py:101-150
        ps = self.ps
        ps.begin_pass()
        x = images if isinstance(images, O.Var) else O.Var(np.asarray(images, dtype=O.DT))
        feats = []
        for l in range(self.levels):
            with ps.variable_scope('unet/encoder/level_%d' % (l + 1)):
                x = self.block(x, self.C * 2 ** l, self.convs)
                feats.append(x)
                x = max_pool2(x)
        with ps.variable_scope('unet/bottom_level'):
            x = self.block(x, self.C * 2 ** self.levels, self.bottom)
        for l in reversed(range(self.levels)):
            with ps.variable_scope('unet/decoder/level_%d' % (l + 1)):
                f = feats[l]
                with ps.variable_scope('up_convolution'):
                    x = O.L_up_convolution(ps, x, f.v.shape[1:-1], 2, [2, 2, 2])
                    x = O.L_batch_norm(ps, x)
                    x = O.L_activation(ps, x, self.act)
                x = self.block2(x, f, self.convs)
        with ps.variable_scope('unet/output'):
            logits = O.L_convolution(ps, x, [1, 1, 1, self.C, self.K])
            logits = O.L_batch_norm(ps, logits)
        return logits

