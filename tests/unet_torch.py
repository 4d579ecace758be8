"""Independent PyTorch-CPU autograd restatement of the reference's U-Net (networks.py:4-150) with torch's own conv3d / max_pool3d /
conv_transpose3d and a batch-norm written by hand, in float64 (the cross-check of tests/unet_oracle.py) or float32 (the yardstick
for what fp32 arithmetic through the network's batch-norms costs against the fp64 oracle).  Variables come from a {TF name: array}
dictionary; forward + soft-Dice (sorensen) loss + backward."""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-3


def _bn(x, gamma, beta):
    ax = (0, 2, 3, 4)
    mu = x.mean(ax, keepdim=True)
    var = ((x - mu) ** 2).mean(ax, keepdim=True)
    return (x - mu) / torch.sqrt(var + EPS) * gamma.view(1, -1, 1, 1, 1) + beta.view(1, -1, 1, 1, 1)


def run(values, x, labels, K, C, levels, convs, bottom, dtype=torch.float64):
    """values: {name: ndarray} (trainables at least); x [B,D,H,W,cin]; labels [B,D,H,W] int.  Returns loss, logits (NDHWC), grads."""
    p = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in values.items()
         if not k.endswith(("moving_mean", "moving_variance"))}
    count = {}

    def bn(scope, t):
        n = count.get(scope, 0)
        count[scope] = n + 1
        base = scope + "/batch_normalization" + ("_%d" % n if n else "")
        return _bn(t, p[base + "/gamma"], p[base + "/beta"])

    def conv(scope, t):
        w = p[scope + "/weights"]                       # DHWIO -> OIDHW
        k = w.shape[0]
        return F.conv3d(t, w.permute(4, 3, 0, 1, 2), p[scope + "/biases"], padding=k // 2)

    def block(scope, t, n):
        for i in range(n):
            s = "%s/conv_%d" % (scope, i + 1)
            t = torch.relu(bn(s, conv(s, t)))
        return t

    t = torch.tensor(np.asarray(x), dtype=dtype).permute(0, 4, 1, 2, 3)
    feats = []
    for l in range(levels):
        t = block("unet/encoder/level_%d" % (l + 1), t, convs)
        feats.append(t)
        t = F.max_pool3d(t, 2, 2)
    t = block("unet/bottom_level", t, bottom)
    for l in reversed(range(levels)):
        s = "unet/decoder/level_%d" % (l + 1)
        w = p[s + "/up_convolution/weights"]            # [2,2,2,Cout,Cin] -> conv_transpose3d weight [Cin,Cout,2,2,2]
        t = F.conv_transpose3d(t, w.permute(4, 3, 0, 1, 2), p[s + "/up_convolution/biases"], stride=2)
        t = torch.relu(bn(s + "/up_convolution", t))
        t = bn(s, torch.cat((t, feats[l]), 1))
        for i in range(convs):
            t = torch.relu(bn(s, conv("%s/conv_%d" % (s, i + 1), t)))
    logits = bn("unet/output", conv("unet/output", t)).permute(0, 2, 3, 4, 1)
    sm = torch.softmax(logits, -1)
    oh = F.one_hot(torch.as_tensor(np.asarray(labels), dtype=torch.int64), K).to(dtype)
    ax = (1, 2, 3)
    inse = (sm * oh).sum(ax)
    dice = ((2.0 * inse + 1e-5) / (sm.sum(ax) + oh.sum(ax) + 1e-5)).mean()     # model.py:26-85 (sorensen), mean over batch and class
    loss = 1.0 - dice
    loss.backward()
    grads = {k: (v.grad.numpy().astype(np.float64) if v.grad is not None else np.zeros(v.shape)) for k, v in p.items()}
    return float(loss.detach()), logits.detach().numpy().astype(np.float64), grads
