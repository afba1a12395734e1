"""One training iteration and one validation pass of the key-point detector: ``train_KPD/src/train.py`` train() / valid()
for the network of ``train_KPD/src/models`` (FastPose_SE: SEResnet with Bottleneck and SELayer, two DUCs, conv_out) under
``torch.optim.RMSprop`` with the hyper-parameters of ``opt.py``.

``TrainableFastPose(device=None)`` runs the host twins of libbetapose_hip.so on numpy arrays (no GPU needed); with a
torch device the kernels of csrc/kpd_train.hip and the GEMM core of csrc/darknet_train.hip run on tensors that stay on
that device.  Convolutions and Linears are the three roles of that core; PyTorch's batch norm with the fused ReLU, the
bottleneck's tail, the SE gate, the max-pool and the RMSprop step are this module's kernels; pixel shuffle is a reshape.
The loss, its gradient and the accuracy are train_data.heatmap_loss_accuracy.  Definitions, declared deviations and the
measured distance from the reference's classes under torch autograd: DESIGN.md 3.14.
"""
from __future__ import annotations

import math

import numpy as np

from . import weights as W

f32 = np.float32
OPT_DEFAULTS = dict(LR=1e-3, momentum=0.0, weightDecay=0.0, alpha=0.99, eps=1e-8)      # train_KPD/src/opt.py, torch's RMSprop


class _Act:
    """an activation and the buffer of its gradient"""

    def __init__(self, v, g):
        self.v, self.g = v, g


class TrainableFastPose:
    """A key-point detector under training.  ``stages`` (``(planes, blocks, stride)`` each) and ``stem`` default to the
    reference's net (weights.fastpose_modules).  ``state_dict``: the reference's keys (a dict of arrays or tensors), or
    None for torch's default initialisation of Conv2d, Linear (``U(-1 / sqrt(fan_in), 1 / sqrt(fan_in))`` for weights and
    biases) and BatchNorm2d (1, 0, running 0 and 1) from numpy's generator with ``seed``: the distributions, not torch's
    bits.  Parameters, gradients, running statistics and the optimiser's state are tensors on ``device``, or numpy arrays
    with ``device=None``."""

    def __init__(self, n_classes=50, stages=W.FASTPOSE_STAGES, stem=64, state_dict=None, device=None, seed=0, LR=OPT_DEFAULTS["LR"],
                 momentum=OPT_DEFAULTS["momentum"], weightDecay=OPT_DEFAULTS["weightDecay"], optMethod="rmsprop", flip_pairs=()):
        from . import _lib
        self._L = _lib
        if optMethod != "rmsprop":
            raise ValueError("optMethod '%s' is not implemented: rmsprop only (adam, sgd and nag are out of scope)" % optMethod)
        self.n_classes, self.stages, self.stem = int(n_classes), tuple(tuple(int(v) for v in s) for s in stages), int(stem)
        self.mods = W.fastpose_modules(self.n_classes, self.stages, self.stem)
        self.hyper = dict(lr=float(LR), momentum=float(momentum), wd=float(weightDecay), alpha=OPT_DEFAULTS["alpha"],
                          eps=OPT_DEFAULTS["eps"])
        self.flip_pairs = tuple(flip_pairs)
        self.side = _lib.Side(device)
        self.torch, self.dev = self.side.torch, self.side.dev
        rng = np.random.default_rng(seed)
        self.P, self.G, self.nbt, self.trainable = {}, {}, {}, []
        self.by_name = {}
        for m in self.mods:
            conv = m["kind"] == "conv"
            k = m["k"] if conv else 1
            shape = (m["cout"], m["cin"], k, k) if conv else (m["cout"], m["cin"])
            bound = 1.0 / math.sqrt(m["cin"] * k * k)
            init = {m["name"] + ".weight": rng.uniform(-bound, bound, shape).astype(f32)}
            if not conv or m["bias"]:
                init[m["name"] + ".bias"] = rng.uniform(-bound, bound, (m["cout"],)).astype(f32)
            bn = m.get("bn") if conv else None
            if bn:
                init.update({bn + ".weight": np.ones(m["cout"], f32), bn + ".bias": np.zeros(m["cout"], f32),
                             bn + ".running_mean": np.zeros(m["cout"], f32), bn + ".running_var": np.ones(m["cout"], f32)})
                self.nbt[bn] = 0
            for key, v in init.items():
                self.P[key] = self._put(v)
                if not key.endswith(("running_mean", "running_var")):
                    self.trainable.append(key)
                    self.G[key] = self._zeros(v.shape)
            self.by_name[m["name"]] = dict(name=m["name"], cin=m["cin"], cout=m["cout"], k=k, stride=m["stride"] if conv else 1, bn=bn)
        self.V = {k: self._zeros(self.P[k].shape) for k in self.trainable}
        self.B = {k: self._zeros(self.P[k].shape) for k in self.trainable}
        self.steps = 0
        self._bufs = {}
        self._table()
        if state_dict is not None:
            self.load_state_dict(state_dict)

    # ------------------------------------------------------------------------------------------- arrays on either side
    def _put(self, a):
        return self.side.put(a, f32, copy=True)      # (the net owns and updates its parameters)

    def _zeros(self, shape, dtype=f32):
        return self.side.zeros(tuple(shape), dtype)

    def _get(self, a):
        return self.side.get(a, copy=True)

    def _buf(self, key, shape, dtype=f32):
        b = self._bufs.get(key)
        if b is None or tuple(b.shape) != tuple(shape):
            b = self._bufs[key] = self._zeros(shape, dtype)
        return b

    def _call(self, name, *args):
        """the host twin, or the device function on the current stream"""
        self.side.call(name, *args)

    def _table(self):
        """the optimiser's table: (parameter, gradient, square_avg, momentum buffer, count) per tensor, on its side"""
        ptr = (lambda a: a.ctypes.data) if self.dev is None else (lambda a: a.data_ptr())
        size = (lambda a: a.size) if self.dev is None else (lambda a: a.numel())
        t = np.array([(ptr(self.P[k]), ptr(self.G[k]), ptr(self.V[k]), ptr(self.B[k]), size(self.P[k])) for k in self.trainable], np.int64)
        chunk = int(self._L.lib().bp_kpd_train_update_chunk())
        self._blocks = int(sum((int(n) + chunk - 1) // chunk for n in t[:, 4]))
        self._tab = t if self.dev is None else self.torch.from_numpy(t).to(self.dev)

    # ------------------------------------------------------------------------------------------- the layers
    def _conv(self, name, a, relu, train):
        """convolution (or Linear: a [N, C] activation is a 1 x 1 map), then batch norm or the bias, then the ReLU"""
        c = self.by_name[name]
        x = a.v
        N, H, Wd = int(x.shape[0]), (int(x.shape[2]) if x.ndim == 4 else 1), (int(x.shape[3]) if x.ndim == 4 else 1)
        k, st, K = c["k"], c["stride"], c["cout"]
        OH, OW = (H + 2 * (k // 2) - k) // st + 1, (Wd + 2 * (k // 2) - k) // st + 1
        shape = (N, K, OH, OW) if x.ndim == 4 else (N, K)
        raw, out, grad = self._buf(name + "/raw", shape), self._buf(name + "/out", shape), self._buf(name + "/grad", shape)
        geom = (N, c["cin"], H, Wd, K, k, st)
        # one scratch for every filter gradient (they run one after the other): the largest any layer needs
        self._scratch = max(self._scratch, int(self._L.lib().bp_kpd_train_conv_scratch(*geom)))
        self._call("bp_kpd_train_conv", 0, x, self.P[name + ".weight"], raw, *geom, None)
        bn = c["bn"]
        if bn:
            mean, invstd = self._buf(name + "/mean", (K,)), self._buf(name + "/invstd", (K,))
            self._call("bp_kpd_train_bn_forward", raw, N, K, OH * OW, self.P[bn + ".weight"], self.P[bn + ".bias"],
                       self.P[bn + ".running_mean"], self.P[bn + ".running_var"], mean, invstd, out, 1, int(relu), int(train))
            if train:
                self.nbt[bn] += 1
        else:
            self._call("bp_kpd_train_bn_forward", raw, N, K, OH * OW, None, self.P[name + ".bias"], None, None, None, None, out, 0,
                       int(relu), 0)
        o = _Act(out, grad)
        self._tape.append(("conv", c, a, o, raw, geom, int(relu)))
        return o

    def _conv_backward(self, c, a, o, raw, geom, relu):
        name, bn = c["name"], c["bn"]
        scratch = self._buf("scratch", (max(self._scratch, 1),))
        N, K = geom[0], geom[4]
        S = int(o.v.shape[2] * o.v.shape[3]) if o.v.ndim == 4 else 1
        if bn:
            self._call("bp_kpd_train_bn_backward", o.v, o.g, raw, self._bufs[name + "/mean"], self._bufs[name + "/invstd"],
                       self.P[bn + ".weight"], N, K, S, self.G[bn + ".weight"], self.G[bn + ".bias"], 1, relu)
        else:
            self._call("bp_kpd_train_bn_backward", o.v, o.g, None, None, None, None, N, K, S, None, self.G[name + ".bias"], 0, relu)
        self._call("bp_kpd_train_conv", 1, a.v, self.G[name + ".weight"], o.g, *geom, scratch)
        if a.g is not None:
            self._call("bp_kpd_train_conv", 2, a.g, self.P[name + ".weight"], o.g, *geom, None)

    def _shuffle(self, a, key):
        """nn.PixelShuffle(2): data movement"""
        x = a.v
        N, C4, H, Wd = (int(v) for v in x.shape)
        if self.dev is None:
            v = np.ascontiguousarray(x.reshape(N, C4 // 4, 2, 2, H, Wd).transpose(0, 1, 4, 2, 5, 3).reshape(N, C4 // 4, 2 * H, 2 * Wd))
        else:
            v = self.torch.nn.functional.pixel_shuffle(x, 2).contiguous()
        o = _Act(v, self._buf(key + "/grad", v.shape))
        self._tape.append(("shuffle", a, o))
        return o

    def _unshuffle(self, a, o):
        g = o.g
        N, C, H2, W2 = (int(v) for v in g.shape)
        if self.dev is None:
            a.g[...] = g.reshape(N, C, H2 // 2, 2, W2 // 2, 2).transpose(0, 1, 3, 5, 2, 4).reshape(N, 4 * C, H2 // 2, W2 // 2)
        else:
            a.g.copy_(self.torch.nn.functional.pixel_unshuffle(g, 2))

    # ------------------------------------------------------------------------------------------- the passes
    def _input(self, inps):
        if self.dev is None:
            x = np.ascontiguousarray(inps.detach().cpu().numpy() if hasattr(inps, "data_ptr") else np.asarray(inps), f32)
        else:
            x = inps if hasattr(inps, "data_ptr") else self.torch.from_numpy(np.ascontiguousarray(inps, f32))
            x = x.to(self.dev, self.torch.float32).contiguous()
        if x.ndim != 4 or x.shape[1] != 3:
            raise ValueError("inps must be [B, 3, H, W]")
        return x

    def forward(self, inps, train=True):
        """``m(inps)``: the heat maps [B, n_classes, H / 4, W / 4] (the net's own buffer: an array, or a tensor on the
        device).  ``train`` uses the batch statistics, updates the running ones and records what backward() needs;
        otherwise the running statistics normalise."""
        self._tape, self._scratch = [], 0
        a = self._conv("preact.conv1", _Act(self._input(inps), None), True, train)
        N, C, H, Wd = (int(v) for v in a.v.shape)
        OH, OW = (H - 1) // 2 + 1, (Wd - 1) // 2 + 1
        p = _Act(self._buf("pool/out", (N, C, OH, OW)), self._buf("pool/grad", (N, C, OH, OW)))
        arg = self._buf("pool/arg", (N, C, OH, OW), np.int32)
        self._call("bp_kpd_train_maxpool_forward", a.v, N * C, H, Wd, p.v, arg)
        self._tape.append(("maxpool", a, p, arg))
        a = p
        for li, (planes, nblocks, stride) in enumerate(self.stages, start=1):
            for bi in range(nblocks):
                pre = "preact.layer%d.%d" % (li, bi)
                x = a
                y = self._conv(pre + ".conv1", x, True, train)
                y = self._conv(pre + ".conv2", y, True, train)
                y = self._conv(pre + ".conv3", y, False, train)
                N, C, H, Wd = (int(v) for v in y.v.shape)
                gate = None
                if pre + ".se.fc.0" in self.by_name:
                    pool = _Act(self._buf(pre + "/pool", (N, C)), self._buf(pre + "/dpool", (N, C)))
                    self._call("bp_kpd_train_pool_forward", y.v, N * C, H * Wd, pool.v)
                    self._tape.append(("pool", y, pool))
                    z = self._conv(pre + ".se.fc.2", self._conv(pre + ".se.fc.0", pool, True, train), False, train)
                    gate = _Act(self._buf(pre + "/gate", (N, C)), z.g)      # the gate's gradient is written where fc.2 reads its own
                    self._call("bp_kpd_train_sigmoid_forward", z.v, gate.v, N * C)
                    self._tape.append(("sigmoid", gate))
                    res = self._conv(pre + ".downsample.0", x, False, train)
                else:
                    res = x
                out = _Act(self._buf(pre + "/out", y.v.shape), self._buf(pre + "/grad", y.v.shape))
                self._call("bp_kpd_train_tail_forward", y.v, None if gate is None else gate.v, res.v, out.v, N, C, H * Wd)
                self._tape.append(("tail", y, gate, res, out))
                a = out
        a = self._shuffle(a, "suffle1")
        a = self._shuffle(self._conv("duc1.conv", a, True, train), "duc1")
        a = self._shuffle(self._conv("duc2.conv", a, True, train), "duc2")
        self._out = self._conv("conv_out", a, False, train)
        return self._out.v

    def backward(self, grad_out):
        """``loss.backward()`` after forward(train=True): ``grad_out`` is the loss's gradient with respect to the heat
        maps; every parameter's gradient is added to (zero_grad() clears them)."""
        seen = set()
        for e in self._tape:        # every activation's gradient starts from zero: the input gradients are added to
            for a in e[1:]:
                if isinstance(a, _Act) and a.g is not None and id(a.g) not in seen:
                    seen.add(id(a.g))
                    a.g[...] = 0
        if self.dev is None:
            self._out.g[...] = np.asarray(grad_out.detach().cpu().numpy() if hasattr(grad_out, "data_ptr") else grad_out, f32)
        else:
            self._out.g.copy_(grad_out if hasattr(grad_out, "data_ptr") else self.torch.from_numpy(np.ascontiguousarray(grad_out, f32)))
        for e in reversed(self._tape):
            kind = e[0]
            if kind == "conv":
                self._conv_backward(*e[1:])
            elif kind == "shuffle":
                self._unshuffle(e[1], e[2])
            elif kind == "tail":
                _, y, gate, res, out = e
                N, C, H, Wd = (int(v) for v in y.v.shape)
                self._call("bp_kpd_train_tail_backward", out.v, out.g, y.v, None if gate is None else gate.v, res.g, y.g,
                           None if gate is None else gate.g, N, C, H * Wd)
            elif kind == "sigmoid":
                g = e[1]
                self._call("bp_kpd_train_sigmoid_backward", g.v, g.g, int(g.v.shape[0] * g.v.shape[1]))
            elif kind == "pool":
                _, y, pool = e
                N, C, H, Wd = (int(v) for v in y.v.shape)
                self._call("bp_kpd_train_pool_backward", pool.g, y.g, N * C, H * Wd)
            else:
                _, a, p, arg = e
                N, C, H, Wd = (int(v) for v in a.v.shape)
                self._call("bp_kpd_train_maxpool_backward", p.g, arg, N * C, H, Wd, a.g)

    def zero_grad(self):
        for g in self.G.values():
            g[...] = 0

    def update(self):
        """``optimizer.step()``: one launch over every parameter tensor"""
        h = self.hyper
        self.steps += 1
        args = (len(self.trainable),) if self.dev is None else (len(self.trainable), self._blocks)
        self._call("bp_kpd_train_rmsprop", self._tab, *args, h["lr"], h["alpha"], h["eps"], h["wd"], h["momentum"])

    def _loss(self, out, labels, set_mask, want_grad):
        """heatmap_loss_accuracy without its read-backs on the device: (loss, acc[0], grad) -- floats on the host, [1]
        tensors on the device"""
        from . import train_data as T
        if self.dev is None:
            loss, acc, _, _, _, grad = T.heatmap_loss_accuracy(out, labels, set_mask, want_grad=want_grad)
            return loss, float(acc[0]), grad
        r = T._loss_call(self.side, out, labels, set_mask, want_grad)
        return r["loss"], r["acc"][:1], r["grad"]

    def _read(self, loss, acc):
        if self.dev is None:
            return float(loss), float(acc)
        v = self.torch.cat([loss, acc.to(self.torch.float64)]).cpu().tolist()      # the one read-back
        return float(v[0]), float(f32(v[1]))

    def train_step(self, inps, labels, set_mask):
        """One iteration of train(): ``out = m(inps)``, ``loss = MSE(out * setMask, labels)``, ``acc`` = accuracy's first
        entry, ``zero_grad``, ``backward``, ``step``.  Returns ``(loss, acc)``, the only values read back."""
        out = self.forward(inps, train=True)
        loss, acc, grad = self._loss(out, labels, set_mask, True)
        self.last_grad_out = grad
        self.zero_grad()
        self.backward(grad)
        self.update()
        return self._read(loss, acc)

    def validate_step(self, inps, labels, set_mask, return_maps=False):
        """One iteration of valid(): forward with the running statistics, the loss of the unflipped pass, then
        ``(flip(shuffleLR(m(flip(inps)))) + out) / 2`` and the accuracy of that.  Returns ``(loss, acc)`` (and the
        averaged maps with ``return_maps``)."""
        from . import train_data as T
        x = self._input(inps)
        B = int(x.shape[0])
        ones, zeros = np.ones(B, np.uint8), np.zeros(B, np.float64)
        out = self.forward(x, train=False)
        out = out.copy() if self.dev is None else out.clone()
        loss, _, _ = self._loss(out, labels, set_mask, False)
        flipped = self.forward(T.augment_maps(x, ones, zeros, (), self.dev), train=False)
        back = T.augment_maps(flipped, ones, zeros, self.flip_pairs, self.dev)
        avg = (back + out) / 2
        _, acc, _ = self._loss(avg, labels, set_mask, False)
        r = self._read(loss, acc)
        return r + (avg,) if return_maps else r

    # ------------------------------------------------------------------------------------------- state, files
    def state_dict(self):
        """The reference's ``m.state_dict()``: its keys in its order as CPU tensors, ``num_batches_tracked`` int64, so
        ``torch.save`` of it is a file the reference, weights.load_kpd_pkl and InferenNet_fast read."""
        import torch
        out = {}
        for m in self.mods:
            n = m["name"]
            out[n + ".weight"] = torch.from_numpy(self._get(self.P[n + ".weight"]))
            if n + ".bias" in self.P:
                out[n + ".bias"] = torch.from_numpy(self._get(self.P[n + ".bias"]))
            bn = m.get("bn")
            if bn:
                for f in ("weight", "bias", "running_mean", "running_var"):
                    out[bn + "." + f] = torch.from_numpy(self._get(self.P[bn + "." + f]))
                out[bn + ".num_batches_tracked"] = torch.tensor(self.nbt[bn], dtype=torch.int64)
        return out

    def _load(self, dst, src, what):
        for k, t in dst.items():
            if k not in src:
                raise ValueError("%s: missing key '%s'" % (what, k))
            v = src[k]
            v = np.ascontiguousarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, f32)
            if v.shape != tuple(t.shape):
                raise ValueError("%s: '%s' has shape %s, the net's is %s" % (what, k, v.shape, tuple(t.shape)))
            t[...] = v if self.dev is None else self.torch.from_numpy(v).to(self.dev)

    def load_state_dict(self, sd):
        self._load(self.P, sd, "state_dict")
        for bn in self.nbt:
            if bn + ".num_batches_tracked" in sd:
                self.nbt[bn] = int(np.asarray(sd[bn + ".num_batches_tracked"]))

    def grads(self):
        return {k: self._get(g) for k, g in self.G.items()}

    def load_grads(self, grads):
        self._load(self.G, grads, "grads")

    def optimizer_state(self):
        """numpy arrays: ``square_avg/<key>`` and ``momentum_buffer/<key>`` per parameter, and ``step``"""
        out = {"step": np.int64(self.steps)}
        for k in self.trainable:
            out["square_avg/" + k] = self._get(self.V[k])
            out["momentum_buffer/" + k] = self._get(self.B[k])
        return out

    def load_optimizer_state(self, st):
        self._load(self.V, {k[len("square_avg/"):]: v for k, v in st.items() if k.startswith("square_avg/")}, "optimizer state")
        self._load(self.B, {k[len("momentum_buffer/"):]: v for k, v in st.items() if k.startswith("momentum_buffer/")}, "optimizer state")
        self.steps = int(st["step"]) if "step" in st else self.steps
