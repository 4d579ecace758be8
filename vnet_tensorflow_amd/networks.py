"""Mirror of the reference's networks.py `class VNet` (networks.py:209-365) -- the network main.py
uses (model.py:428-438) -- wired onto the fused HIP ops.

Same constructor signature / defaults, same `GetNetwork(x)` entry point, same TF variable names
(SURVEY.md B.1).  Differences that do not change results: the channel concat (networks.py:325)
is never materialised (the conv reads two sources), tf.tile of the 1-channel input
(networks.py:258), the residual adds (networks.py:318,336,360) and the activation are fused
into the batch-norm kernels.  `train_phase` is kept as an attribute for API parity; like the
reference (which feeds True in train, test and evaluate, model.py:747,788,917) batch statistics
are always used.
"""
import torch

from . import layers2 as L
from ._scope import VariableStore


class VNet(object):
    def __init__(self,
                 num_classes,
                 dropout_rate=0.01,
                 num_channels=16,
                 num_levels=4,
                 num_convolutions=(1, 2, 3, 3),
                 bottom_convolutions=3,
                 is_training=True,
                 activation_fn="relu",
                 device=None):
        """Implements VNet architecture https://arxiv.org/abs/1606.04797 (reference networks.py:210-244)."""
        self.num_classes = num_classes
        self.dropout_rate = dropout_rate
        self.num_channels = num_channels
        assert num_levels == len(num_convolutions)
        self.num_levels = num_levels
        self.num_convolutions = num_convolutions
        self.bottom_convolutions = bottom_convolutions
        self.is_training = is_training
        self.train_phase = True            # stand-in for the "train_phase_placeholder" (networks.py:237)
        if activation_fn not in ("relu", "prelu", "lrelu"):
            raise ValueError("activation_fn must be relu, prelu or lrelu")
        self.activation_fn = activation_fn
        self.fuse_input_block = True       # single-modality input: skip the 16x redundant work of the tiled conv
        self.fuse_bn_chains = True         # decoder BN->BN->add->BN chains in closed form (ops.bn_chain)
        self.cut_backward = False          # data-parallel step graphs: cut the autograd graph between encoder and bottom level / skips
        self.backward_cuts = []
        self.fuse_bn_stats = True          # batch-norm statistics from the producing convolution's epilogue (ops.conv bn_stats)
        self.fuse_grad_accumulation = True # tensors with two consumers: second gradient accumulated by its producer (ops.fork)
        self.fuse_zero_bias_grad = True    # conv biases feed batch-norms: their gradient is identically 0 (ops.zero_bias_gradients)
        self.fuse_head = True              # the 1x1x1 output convolution runs inside the decoder's last batch-norm passes (ops.bn_head)
        self.variables = VariableStore(device)

    # -- torch.nn.Module-like conveniences -------------------------------------------------
    def parameters(self):
        return list(self.variables.params.values())

    def named_parameters(self):
        return list(self.variables.params.items())

    def state_dict(self):
        return self.variables.state_dict()

    def load_state_dict(self, sd):
        self.variables.load_state_dict(sd)

    def build(self, input_shape):
        """Create all variables (on self.variables.device) from a shape only -- replaces the
        graph-construction pass of TF (model.py:444)."""
        with torch.no_grad():
            self.GetNetwork(torch.empty(tuple(input_shape), device="meta"))
        return self

    def _dropout_rate(self):
        r = self.dropout_rate if self.is_training else 0.0
        return float(r() if callable(r) else r)

    # -- reference networks.py:246-305 ---------------------------------------------------------
    def GetNetwork(self, x):
        store = self.variables
        if store.device is None and x.device.type != "meta":
            store.device = x.device
        store.begin_pass()
        dropout_rate = self._dropout_rate()
        act = self.activation_fn
        from . import ops
        with store.active(), ops.zero_bias_gradients(self.fuse_zero_bias_grad):
            if x.dim() != 5:
                raise NotImplementedError("only 3-D PatchShape is built (2-D is out of scope, SURVEY section 2 row 11)")
            input_channels = int(x.shape[-1])
            with store.variable_scope('vnet/input_layer'):
                tiled = None
                store16 = ops.storage_is_bf16() and x.device.type != "meta"
                if store16 and (self.num_channels < 8 or self.num_channels & (self.num_channels - 1)):
                    raise ops.VnetHipError("ComputeDtype 'bf16' stores activations as bf16 in 16-byte channel units: NumChannel must be "
                                           "8 * 2^k (got %d); use 'fp32' or 'fp32_split3'" % self.num_channels)
                if input_channels == 1:
                    # tile + BN; the first 5^3 conv then runs on the un-tiled image (layers2.convolution_tiled)
                    x, tiled = L.batch_normalization(x, tile=True, channels=self.num_channels, want_stats=True)
                    if self.num_channels > 16 or not self.fuse_input_block or store16:
                        tiled = None          # (bf16 storage: the tiled batch-norm writes a bf16 tensor, conv_1 is an ordinary bf16 conv)
                else:
                    if store16:
                        x = ops.cast_input(x)     # bf16, channels zero-padded to the 16-byte unit; from here on every tensor is bf16
                    x = L.convolution(x, [5, 5, 5, input_channels, self.num_channels], bn_stats=self.fuse_bn_stats)
                    x = L.batch_normalization(x, activation=act)

            features = list()
            cutting = self.cut_backward and x.device.type != "meta" and torch.is_grad_enabled()
            self.backward_cuts = []
            for l in range(self.num_levels):
                with store.variable_scope('vnet/encoder/level_' + str(l + 1)):
                    x = self.convolution_block(x, self.num_convolutions[l], dropout_rate, act,
                                               tiled=tiled if l == 0 else None)
                    if self.fuse_grad_accumulation and not cutting:
                        # skip connection: decoder concat + down convolution consume x (ops.fork)
                        skip, x = ops.fork(x)
                        features.append(skip)
                    else:
                        features.append(x)
                    with store.variable_scope('down_convolution'):
                        x = L.down_convolution(x, factor=2, kernel_size=[2, 2, 2], bn_stats=self.fuse_bn_stats)
                        x = L.batch_normalization(x, activation=act)

            if cutting:
                # everything the decoder and the bottom level take from the encoder becomes a leaf: backward pass 1 ends here
                features = [ops.cut(f, self.backward_cuts) for f in features]
                x = ops.cut(x, self.backward_cuts)
            with store.variable_scope('vnet/bottom_level'):
                x = self.convolution_block(x, self.bottom_convolutions, dropout_rate, act)

            for l in reversed(range(self.num_levels)):
                with store.variable_scope('vnet/decoder/level_' + str(l + 1)):
                    f = features[l]
                    with store.variable_scope('up_convolution'):
                        x = L.up_convolution(x, tuple(f.shape), factor=2, kernel_size=[2, 2, 2])
                        x = L.batch_normalization(x, activation=act)
                    x = self.convolution_block_2(x, f, self.num_convolutions[l], dropout_rate, act,
                                                 head=(l == 0 and self.fuse_head))

            with store.variable_scope('vnet/output_layer'):
                if isinstance(x, L.DeferredNorm):
                    # the block's last batch-norm has not run: it and the 1x1x1 convolution share their passes
                    logits = L.convolution_after_norm(x, [1, 1, 1, self.num_channels, self.num_classes])
                else:
                    logits = L.convolution(x, [1, 1, 1, self.num_channels, self.num_classes])
                logits = L.batch_normalization(logits)
        return logits

    # -- reference networks.py:307-322 ---------------------------------------------------------
    def convolution_block(self, layer_input, num_convolutions, dropout_rate, activation_fn, is_training=True, tiled=None):
        from . import ops
        store = self.variables
        x = layer_input
        n_channels = L.get_num_channels(x)
        if tiled is None and self.fuse_grad_accumulation:
            # the block input feeds conv_1 and the residual add: its second gradient is accumulated in place (ops.fork)
            x, layer_input = ops.fork(layer_input)
        for i in range(num_convolutions):
            with store.variable_scope('conv_' + str(i + 1)):
                res = layer_input if i == num_convolutions - 1 else None          # x = x + layer_input
                if i == 0 and tiled is not None:
                    x = L.convolution_tiled(tiled, [5, 5, 5, n_channels, n_channels], bn_stats=self.fuse_bn_stats, bn_residual=res)
                else:
                    x = L.convolution(x, [5, 5, 5, n_channels, n_channels], bn_stats=self.fuse_bn_stats, bn_residual=res)
                x = L.batch_normalization(x, activation=activation_fn, residual=res)
                x = ops.dropout(x, dropout_rate)
        return x

    # -- reference networks.py:324-365 ---------------------------------------------------------
    def convolution_block_2(self, layer_input, fine_grained_features, num_convolutions, dropout_rate, activation_fn,
                            is_training=True, head=False):
        """head: the block's output feeds only the 1x1x1 output convolution -- with no dropout in between its last batch-norm is
        returned un-run (layers2.DeferredNorm) for the output layer to fold the convolution into."""
        from . import ops
        store = self.variables
        n_channels = L.get_num_channels(layer_input)
        defer = bool(head) and dropout_rate == 0.0
        if num_convolutions == 1:
            with store.variable_scope('conv_' + str(1)):
                x = L.convolution_concat(layer_input, fine_grained_features, [5, 5, 5, n_channels * 2, n_channels], bn_stats=self.fuse_bn_stats)
                if self.fuse_bn_chains:
                    # x = BN(x); r = BN(x) (networks.py:335); x = act(BN(x + r)) -- one fused normalisation of the conv output
                    x = L.batch_normalization_chain(x, 0, activation_fn, defer=defer)
                else:
                    x = L.batch_normalization(x)
                    r = L.batch_normalization(x)                                       # networks.py:335
                    x = L.batch_normalization(x, activation=activation_fn, residual=r, defer=defer)  # x = x + layer_input ; BN ; act
                if not defer:
                    x = ops.dropout(x, dropout_rate)
            return x

        with store.variable_scope('conv_' + str(1)):
            x = L.convolution_concat(layer_input, fine_grained_features, [5, 5, 5, n_channels * 2, n_channels], bn_stats=self.fuse_bn_stats)
            x = L.batch_normalization(x, activation=activation_fn)
            x = ops.dropout(x, dropout_rate)

        for i in range(1, num_convolutions):
            with store.variable_scope('conv_' + str(i + 1)):
                x = L.convolution(x, [5, 5, 5, n_channels, n_channels], bn_stats=self.fuse_bn_stats)
                last = (i == num_convolutions - 1)
                # networks.py:358 builds this BN for every i; its output is used only by the last conv
                if last and self.fuse_bn_chains:
                    x = L.batch_normalization_chain(x, 1, activation_fn, defer=defer)  # r = BN(x); x = act(BN(x + r))
                else:
                    r = L.batch_normalization(x, dead=not last)
                    x = L.batch_normalization(x, activation=activation_fn, residual=r if last else None, defer=defer and last)
                if not (defer and last):
                    x = ops.dropout(x, dropout_rate)
        return x


class UNet(object):
    """Mirror of the reference's `class UNet` (networks.py:4-150), the network model.py:414-427 builds for
    `Networks.Name == "UNet"`: 3x3x3 SAME convolutions, 2x2x2 VALID max-pooling, 2x2x2 transposed up-convolutions, one batch-norm
    over each decoder concat.  Same constructor signature / defaults, `GetNetwork(x)`, and TF variable names in creation order
    ('unet/encoder/level_1/conv_1/weights', ..., 'unet/decoder/level_1/batch_normalization_2/gamma', 'unet/output/...': the
    decoder block's batch-norms sit OUTSIDE its conv_i scopes, networks.py:65,84).  Differences that do not change results: the
    concat is never materialised (its batch-norm runs on the two halves, the convolution behind reads two sources) and the
    activation is fused into the batch-norm kernels.  Batch statistics are always used, like the reference (model.py:747,788,917).
    ComputeDtype 'fp32' and 'fp32_split3' both run it on the fp32 MFMA kernels (the f32x3 kernels are 5^3 only); 'bf16' is refused."""

    def __init__(self,
                 num_output_channels,
                 dropout_rate=0.01,
                 num_channels=4,
                 num_levels=4,
                 num_convolutions=2,
                 bottom_convolutions=2,
                 is_training=True,
                 activation_fn="relu",
                 device=None):
        self.num_output_channels = num_output_channels
        self.dropout_rate = dropout_rate
        self.num_channels = num_channels
        self.num_levels = num_levels
        for what, n in (("num_convolutions", num_convolutions), ("bottom_convolutions", bottom_convolutions)):
            if isinstance(n, bool) or not isinstance(n, int):
                raise ValueError("UNet: %s is one integer for every level (reference networks.py:10-11), got %r" % (what, n))
        self.num_convolutions = num_convolutions
        self.bottom_convolutions = bottom_convolutions
        self.is_training = is_training
        self.train_phase = True            # stand-in for the "train_phase_placeholder" (networks.py:32)
        if activation_fn not in ("relu", "prelu", "lrelu"):
            raise ValueError("activation_fn must be relu, prelu or lrelu")
        self.activation_fn = activation_fn
        self.fuse_bn_stats = True          # batch-norm statistics from the producing convolution's epilogue (ops.conv bn_stats)
        self.fuse_grad_accumulation = True # skip features have two consumers: the second gradient is accumulated in place (ops.fork)
        self.fuse_zero_bias_grad = True    # every conv feeds a batch-norm: its bias gradient is identically 0 (ops.zero_bias_gradients)
        self.variables = VariableStore(device)

    parameters = VNet.parameters
    named_parameters = VNet.named_parameters
    state_dict = VNet.state_dict
    load_state_dict = VNet.load_state_dict
    build = VNet.build
    _dropout_rate = VNet._dropout_rate

    # -- reference networks.py:41-61 -----------------------------------------------------------
    def convolution_block(self, layer_input, output_channel, num_convolutions, dropout_rate, activation_fn, is_training=True):
        from . import ops
        store = self.variables
        x = layer_input
        input_channels = L.get_num_channels(x)
        for i in range(num_convolutions):
            with store.variable_scope('conv_' + str(i + 1)):
                x = L.convolution(x, [3, 3, 3, input_channels if i == 0 else output_channel, output_channel], bn_stats=self.fuse_bn_stats)
                x = L.batch_normalization(x, activation=activation_fn)
                x = ops.dropout(x, dropout_rate)
        return x

    # -- reference networks.py:63-99 -----------------------------------------------------------
    def convolution_block_2(self, layer_input, fine_grained_features, num_convolutions, dropout_rate, activation_fn,
                            is_training=True):
        from . import ops
        store = self.variables
        num_channels = L.get_num_channels(layer_input)
        # x = BN(concat(layer_input, features)): per channel, so the two halves are normalised on their own (one variable set)
        x, skip = L.batch_normalization_concat(layer_input, fine_grained_features)
        for i in range(num_convolutions):
            with store.variable_scope('conv_' + str(i + 1)):
                if i == 0:
                    x = L.convolution_concat(x, skip, [3, 3, 3, num_channels + L.get_num_channels(skip), num_channels],
                                             bn_stats=self.fuse_bn_stats)
                else:
                    x = L.convolution(x, [3, 3, 3, num_channels, num_channels], bn_stats=self.fuse_bn_stats)
            x = L.batch_normalization(x, activation=activation_fn)     # (outside the conv_i scope: networks.py:84)
            x = ops.dropout(x, dropout_rate)
        return x

    # -- reference networks.py:101-150 ---------------------------------------------------------
    def GetNetwork(self, x):
        from . import ops
        store = self.variables
        if store.device is None and x.device.type != "meta":
            store.device = x.device
        store.begin_pass()
        dropout_rate = self._dropout_rate()
        act = self.activation_fn
        if x.dim() != 5:
            raise NotImplementedError("only 3-D PatchShape is built (2-D is out of scope, SURVEY section 2 row 11)")
        if ops.storage_is_bf16() and x.device.type != "meta":
            raise ops.VnetHipError("ComputeDtype 'bf16' with Networks.Name 'UNet' is not built (the bf16-storage kernels are the "
                                   "V-Net's 5^3 / 2^3 set); use 'fp32' or 'fp32_split3'")
        with store.active(), ops.zero_bias_gradients(self.fuse_zero_bias_grad):
            features = list()
            for l in range(self.num_levels):
                with store.variable_scope('unet/encoder/level_' + str(l + 1)):
                    x = self.convolution_block(x, self.num_channels * (2 ** l), self.num_convolutions, dropout_rate, act)
                    if self.fuse_grad_accumulation:
                        skip, x = ops.fork(x)          # skip connection: the decoder's concat batch-norm + the max-pooling consume x
                        features.append(skip)
                    else:
                        features.append(x)
                    if any(int(v) % 2 for v in x.shape[1:4]):
                        # VALID pooling floors, the SAME transposed convolution back needs ceil(fine / 2) coarse voxels: TF 1.15
                        # refuses the reference's graph here (conv3d_transpose: "out_backprop doesn't match computed"), so do we
                        raise ops.VnetHipError("UNet: level %d has the odd size %s -- every PatchShape axis must be a multiple of "
                                               "2^NumLevels (the reference's max_pool3d VALID / conv3d_transpose SAME pair does not "
                                               "build otherwise)" % (l + 1, tuple(int(v) for v in x.shape[1:4])))
                    with store.variable_scope('max_pooling'):
                        x = L.max_pool3d(x, ksize=[1, 2, 2, 2, 1], strides=[1, 2, 2, 2, 1], padding='VALID')

            with store.variable_scope('unet/bottom_level'):
                x = self.convolution_block(x, self.num_channels * (2 ** self.num_levels), self.bottom_convolutions, dropout_rate, act)

            for l in reversed(range(self.num_levels)):
                with store.variable_scope('unet/decoder/level_' + str(l + 1)):
                    f = features[l]
                    with store.variable_scope('up_convolution'):
                        x = L.up_convolution(x, tuple(f.shape), factor=2, kernel_size=[2, 2, 2])
                        x = L.batch_normalization(x, activation=act)
                        x = ops.dropout(x, dropout_rate)
                    x = self.convolution_block_2(x, f, self.num_convolutions, dropout_rate, act)

            with store.variable_scope('unet/output'):
                logits = L.convolution(x, [1, 1, 1, self.num_channels, self.num_output_channels])
                logits = L.batch_normalization(logits)
        return logits
