"""The training iteration of DESIGN.md 3.13 restated in float64 numpy: the one text the fixture maker
(tools/make_golden_darknet_train.py) forms its bars with and the tests of the shipped topology compare against.  It
reads nothing of the reference."""
import numpy as np

from betapose_amd.darknet_train import learning_rate
from betapose_amd.yolo_train import yolo_loss

f32, f64 = np.float32, np.float64


class F64Net:
    """forward with batch statistics, backward and update of DESIGN.md 3.13 in float64"""

    def __init__(self, net, layers, st, blas=False):
        """``blas`` lets einsum hand its contractions to the BLAS (another order of summation, in float64 still): what
        the 75-convolution net needs; the tiny nets' bars were formed without"""
        self.net, self.layers, self.blas = net, layers, blas
        self.convs = [l for l in layers if l["type"] == "convolutional"]
        self.st = {k: v.astype(f64) for k, v in st.items()}
        for n, l in enumerate(self.convs):
            for k, src in (("weight_updates", "weights"), ("bias_updates", "biases"), ("scale_updates", "scales")):
                if "conv%d.%s" % (n, src) in self.st:
                    self.st.setdefault("conv%d.%s" % (n, k), np.zeros_like(self.st["conv%d.%s" % (n, src)]))
        self.seen = 0

    @staticmethod
    def cols(x, s, stride):
        p = s // 2
        N, c, H, W = x.shape
        OH, OW = (H + 2 * p - s) // stride + 1, (W + 2 * p - s) // stride + 1
        xp = np.pad(x, ((0, 0), (0, 0), (p, p), (p, p)))
        return np.stack([xp[:, :, ky:ky + stride * OH:stride, kx:kx + stride * OW:stride] for ky in range(s) for kx in range(s)], 2)

    def forward(self, x):
        x = x.astype(f64)
        self.inp, outs, heads, rec, n = x, [], [], {}, 0
        for l in self.layers:
            t = l["type"]
            if t == "convolutional":
                p = "conv%d." % n
                w = self.st[p + "weights"]
                K, c, s = w.shape[:3]
                l["cols"] = self.cols(x, s, l["stride"])
                raw = np.einsum("nctyx,kct->nkyx", l["cols"], w.reshape(K, c, s * s), optimize=self.blas)
                if l["bn"]:
                    cnt = raw.shape[0] * raw.shape[2] * raw.shape[3]
                    mean = raw.mean((0, 2, 3))
                    var = ((raw - mean[None, :, None, None]) ** 2).sum((0, 2, 3)) / (cnt - 1)
                    for k, v in (("rolling_mean", mean), ("rolling_variance", var)):
                        self.st[p + k] = .9 * self.st[p + k] + .1 * v
                    xn = (raw - mean[None, :, None, None]) / (np.sqrt(var) + 1e-6)[None, :, None, None]
                    l.update(x=raw, x_norm=xn, mean=mean, var=var)
                    rec[p + "mean"], rec[p + "variance"] = mean, var
                    raw = xn * self.st[p + "scales"][None, :, None, None]
                raw = raw + self.st[p + "biases"][None, :, None, None]
                x = np.where(raw > 0, raw, .1 * raw) if l["leaky"] else raw
                rec[p + "output"] = x
                n += 1
            elif t == "shortcut":
                x = x + outs[l["src"]]
            elif t == "route":
                x = np.concatenate([outs[s] for s in l["src"]], 1)
            elif t == "upsample":
                x = x.repeat(2, 2).repeat(2, 3)
            else:
                heads.append(x)
            outs.append(x)
        self.outs = outs
        return heads, rec

    def masks(self):
        """after forward: per convolution, where its leaky output is positive (None for a linear one)"""
        return [self.outs[i] > 0 if l["leaky"] else None for i, l in enumerate(self.layers) if l["type"] == "convolutional"]

    def backward(self, head_deltas, masks=None):
        """``masks``: per convolution the leaky mask (output > 0) of the run this one is compared with, in place of
        this run's own: the gradient is discontinuous at 0, and where a pre-activation lies closer to 0 than float32
        resolves, a flipped element is an error of neither side."""
        deltas = [np.zeros_like(o) for o in self.outs]
        hd, n = list(head_deltas), len(self.convs)
        for i in range(len(self.layers) - 1, -1, -1):
            l, t, d = self.layers[i], self.layers[i]["type"], deltas[i]
            if t == "yolo":
                deltas[i - 1] += hd.pop().astype(f64)
            elif t == "convolutional":
                n -= 1
                p = "conv%d." % n
                pos = self.outs[i] > 0 if masks is None or masks[n] is None else np.asarray(masks[n], bool)
                d = d * np.where(pos, 1.0, .1) if l["leaky"] else d
                self.st[p + "bias_updates"] += d.sum((0, 2, 3))
                if l["bn"]:
                    cnt = d.shape[0] * d.shape[2] * d.shape[3]
                    mean, var = l["mean"][None, :, None, None], l["var"][None, :, None, None]
                    self.st[p + "scale_updates"] += (d * l["x_norm"]).sum((0, 2, 3))
                    d = d * self.st[p + "scales"][None, :, None, None]
                    md = d.sum((0, 2, 3), keepdims=True) * (-1. / np.sqrt(var + 1e-5))
                    vd = (d * (l["x"] - mean)).sum((0, 2, 3), keepdims=True) * -.5 * (var + 1e-5) ** -1.5
                    d = d / (np.sqrt(var) + 1e-5) + vd * 2. * (l["x"] - mean) / cnt + md / cnt
                w = self.st[p + "weights"]
                K, c, s = w.shape[:3]
                self.st[p + "weight_updates"] += np.einsum("nkyx,nctyx->kct", d, l["cols"], optimize=self.blas).reshape(w.shape)
                if i:
                    dc = np.einsum("nkyx,kct->nctyx", d, w.reshape(K, c, s * s), optimize=self.blas)
                    pd, st = s // 2, l["stride"]
                    N, _, H, W = deltas[i - 1].shape
                    OH, OW = d.shape[2:]
                    buf = np.zeros((N, c, H + 2 * pd, W + 2 * pd))
                    for ky in range(s):
                        for kx in range(s):
                            buf[:, :, ky:ky + st * OH:st, kx:kx + st * OW:st] += dc[:, :, ky * s + kx]
                    deltas[i - 1] += buf[:, :, pd:pd + H, pd:pd + W]
            elif t == "shortcut":
                deltas[i - 1] += d
                deltas[l["src"]] += d
            elif t == "route":
                at = 0
                for s_ in l["src"]:
                    c = self.outs[s_].shape[1]
                    deltas[s_] += d[:, at:at + c]
                    at += c
            elif t == "upsample":
                deltas[i - 1] += d[:, :, 0::2, 0::2] + d[:, :, 0::2, 1::2] + d[:, :, 1::2, 0::2] + d[:, :, 1::2, 1::2]

    def update(self):
        ub = self.net["batch"] * self.net["subdivisions"]
        rate = float(learning_rate(self.net, self.seen // ub))
        mom, decay = float(self.net["momentum"]), float(self.net["decay"])
        for n, l in enumerate(self.convs):
            p = "conv%d." % n
            for k, u in (("biases", "bias_updates"), ("scales", "scale_updates"), ("weights", "weight_updates")):
                if p + k not in self.st:
                    continue
                if k == "weights":
                    self.st[p + u] = self.st[p + u] - decay * ub * self.st[p + k]
                self.st[p + k] = self.st[p + k] + rate / ub * self.st[p + u]
                self.st[p + u] = self.st[p + u] * mom

    def step(self, x, head_deltas=None, truth=None, masks=None):
        """one train_network_datum: (cost, the forward's record, the update buffers before the update)"""
        self.seen += self.net["batch"]
        heads, rec = self.forward(x)
        costs = None
        if head_deltas is None:
            head_deltas, costs = [], []
            for l, h in zip([l for l in self.layers if l["type"] == "yolo"], heads):
                p = l["head"]
                c, _, d, _ = yolo_loss(h.astype(f32), truth, (self.net["height"], self.net["width"]), p["anchors"], p["mask"], p["classes"],
                                       p["ignore_thresh"], p["truth_thresh"], want_act=False)
                head_deltas.append(d), costs.append(c)
        self.backward(head_deltas, masks)
        pre = {k: v.copy() for k, v in self.st.items() if k.endswith("_updates")}
        if (self.seen // self.net["batch"]) % self.net["subdivisions"] == 0:
            self.update()
        return (None if costs is None else float(np.mean(costs))), rec, pre


def mask_flips(masks, free):
    """(leaky outputs whose sign differs between two runs' masks, leaky outputs in all)"""
    pairs = [(np.asarray(a, bool), b) for a, b in zip(masks, free) if b is not None]
    return int(sum(np.count_nonzero(a != b) for a, b in pairs)), int(sum(b.size for _, b in pairs))
