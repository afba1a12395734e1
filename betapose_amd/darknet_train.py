"""One training iteration of ``./darknet detector train``: Darknet's forward pass with batch statistics, its backward
pass and its momentum / decay update (``train_YOLO/src/network.c`` train_network_datum, ``convolutional_layer.c``,
``batchnorm_layer.c``, ``blas.c``, ``shortcut_layer.c``, ``route_layer.c``, ``upsample_layer.c``), for the layer set
the reference's two cfgs emit.

``TrainableDarknet(cfg, device=None)`` runs the host twins of libbetapose_hip.so on numpy arrays (no GPU needed); with
a torch device the kernels of csrc/darknet_train.hip run on tensors that stay on that device: the convolution's three
GEMMs on the fp32 matrix pipe, the batch-norm reductions, and one launch that updates every parameter.  Shortcut, route
and upsample are slices and adds.  The heads are yolo_train.yolo_loss.  Definitions, declared deviations and the
measured distance from the reference's C code: DESIGN.md 3.13.
"""
from __future__ import annotations

import math

import numpy as np

from . import cfg as C, weights as W
from .yolo_train import _loss_call, yolo_head_params, yolo_loss

f32 = np.float32
POLICIES = ("constant", "steps", "step", "exp", "poly")
_NET_KEYS = {"type", "batch", "subdivisions", "width", "height", "channels", "momentum", "decay", "learning_rate", "burn_in", "power",
             "policy", "steps", "scales", "step", "scale", "gamma", "max_batches", "jitter", "hue", "saturation", "exposure", "angle",
             "flip", "small_object"}
_CONV_KEYS = {"type", "batch_normalize", "filters", "size", "stride", "pad", "activation"}
_YOLO_KEYS = {"type", "mask", "anchors", "classes", "num", "jitter", "ignore_thresh", "truth_thresh", "random", "max"}


def _bad(key, why):
    raise ValueError("unsupported cfg key '%s': %s" % (key, why))


def net_options(block):
    """parse_net_options for the keys this module reads: a dict; the net's batch is ``batch / subdivisions``."""
    for k in block:
        if k not in _NET_KEYS:
            _bad(k, "not read by the [net] section here")
    if float(block.get("angle", 0)) != 0:
        _bad("angle", "rotation is not implemented")
    sub = int(block.get("subdivisions", 1))
    o = dict(batch=int(block.get("batch", 1)) // sub, subdivisions=sub, width=int(block.get("width", 0)),
             height=int(block.get("height", 0)), channels=int(block.get("channels", 0)),
             momentum=f32(block.get("momentum", .9)), decay=f32(block.get("decay", .0001)),
             learning_rate=f32(block.get("learning_rate", .001)), burn_in=int(block.get("burn_in", 0)),
             power=f32(block.get("power", 4)), policy=block.get("policy", "constant"), max_batches=int(block.get("max_batches", 0)),
             jitter=float(block.get("jitter", .2)), hue=float(block.get("hue", 0)), saturation=float(block.get("saturation", 1)),
             exposure=float(block.get("exposure", 1)))
    if o["policy"] not in POLICIES:
        _bad("policy", "'%s' is not one of %s" % (o["policy"], ", ".join(POLICIES)))
    if o["batch"] < 1 or o["width"] < 1 or o["height"] < 1 or o["channels"] < 1:
        raise ValueError("[net] needs batch >= subdivisions, width, height and channels")
    if o["policy"] == "step":
        o["step"], o["scale"] = int(block.get("step", 1)), f32(block.get("scale", 1))
    elif o["policy"] == "steps":
        if "steps" not in block or "scales" not in block:
            raise ValueError("the steps policy needs steps and scales")
        o["steps"] = [int(v) for v in block["steps"].split(",")]
        o["scales"] = [f32(v) for v in block["scales"].split(",")][:len(o["steps"])]
        if len(o["scales"]) != len(o["steps"]):
            raise ValueError("steps and scales differ in length")
    elif o["policy"] == "exp":
        o["gamma"] = f32(block.get("gamma", 1))
    return o


def learning_rate(net, batch_num):
    """get_current_rate (network.c:89-122) at ``batch_num`` = seen / (batch * subdivisions), a float32: the float
    operands, C's ``pow`` in double, the product in double, rounded once."""
    lr, n = f32(net["learning_rate"]), int(batch_num)
    if n < net["burn_in"]:
        return f32(float(lr) * math.pow(float(f32(n) / f32(net["burn_in"])), float(net["power"])))
    p = net["policy"]
    if p == "constant":
        return lr
    if p == "step":
        return f32(float(lr) * math.pow(float(net["scale"]), n // net["step"]))
    if p == "steps":
        rate = lr
        for s, k in zip(net["steps"], net["scales"]):
            if s > n:
                return rate
            rate = f32(rate * k)
        return rate
    if p == "exp":
        return f32(float(lr) * math.pow(float(net["gamma"]), n))
    if p == "poly":
        return f32(float(lr) * math.pow(float(f32(1) - f32(n) / f32(net["max_batches"])), float(net["power"])))
    _bad("policy", p)


def parse_layers(blocks):
    """The layers of a parsed cfg after [net] as dicts with their output shapes (c, h, w); anything outside the
    supported set raises ValueError naming the key (or the section)."""
    net = net_options(blocks[0]) if blocks and blocks[0]["type"] == "net" else _bad("net", "the cfg must begin with [net]")
    layers, shape = [], (net["channels"], net["height"], net["width"])
    for b in blocks[1:]:
        t, i = b["type"], len(layers)
        if t == "convolutional":
            for k in b:
                if k not in _CONV_KEYS:
                    _bad(k, "not supported in [convolutional]")
            size, stride, act = int(b.get("size", 1)), int(b.get("stride", 1)), b.get("activation", "logistic")
            if size not in (1, 3):
                _bad("size", "1 or 3 only")
            if stride not in (1, 2):
                _bad("stride", "1 or 2 only")
            if int(b.get("pad", 0)) != 1 and size != 1:
                _bad("pad", "pad=1 (padding size / 2) only")
            if act not in ("leaky", "linear"):
                _bad("activation", "leaky or linear only, not %s" % act)
            pad = size // 2
            out = (int(b["filters"]), (shape[1] + 2 * pad - size) // stride + 1, (shape[2] + 2 * pad - size) // stride + 1)
            layers.append(dict(type=t, cin=shape[0], size=size, stride=stride, bn=int(b.get("batch_normalize", 0)) > 0,
                               leaky=int(act == "leaky"), inp=shape, out=out))
        elif t == "shortcut":
            for k in b:
                if k not in ("type", "from", "activation"):
                    _bad(k, "not supported in [shortcut]")
            if b.get("activation", "linear") != "linear":
                _bad("activation", "a shortcut is linear here")
            src = int(b["from"])
            src = src + i if src < 0 else src
            if not 0 <= src < i or layers[src]["out"] != shape:
                _bad("from", "the shortcut's source must be an earlier layer of the same shape")
            layers.append(dict(type=t, src=src, out=shape))
        elif t == "route":
            for k in b:
                if k not in ("type", "layers"):
                    _bad(k, "not supported in [route]")
            src = [int(v) for v in b["layers"].split(",")]
            src = [s + i if s < 0 else s for s in src]
            if not 1 <= len(src) <= 2 or any(not 0 <= s < i for s in src) or len({layers[s]["out"][1:] for s in src}) != 1:
                _bad("layers", "a route takes 1 or 2 earlier layers of one spatial size")
            layers.append(dict(type=t, src=src, out=(sum(layers[s]["out"][0] for s in src),) + layers[src[0]]["out"][1:]))
        elif t == "upsample":
            for k in b:
                if k not in ("type", "stride"):
                    _bad(k, "not supported in [upsample]")
            if int(b.get("stride", 2)) != 2:
                _bad("stride", "an upsample has stride 2 here")
            layers.append(dict(type=t, out=(shape[0], shape[1] * 2, shape[2] * 2)))
        elif t == "yolo":
            for k in b:
                if k not in _YOLO_KEYS:
                    _bad(k, "not supported in [yolo]")
            if int(b.get("random", 0)):
                _bad("random", "multi-scale training (random=1) is not implemented")
            layers.append(dict(type=t, out=shape, head=yolo_head_params([b])[0]))
            h = layers[-1]["head"]
            if len(h["mask"]) * (5 + h["classes"]) != shape[0]:
                raise ValueError("a [yolo] block expects %d channels, the layer before it has %d"
                                 % (len(h["mask"]) * (5 + h["classes"]), shape[0]))
        else:
            _bad(t, "section not supported")
        shape = layers[-1]["out"]
    if not any(l["type"] == "yolo" for l in layers):
        raise ValueError("the cfg has no [yolo] layer")
    return net, layers


_PARAMS = ("biases", "scales", "rolling_mean", "rolling_variance", "weights")
_UPDATES = ("bias_updates", "scale_updates", "weight_updates")


class TrainableDarknet:
    """A detector under training.  ``weights``: a .weights file (its ``seen`` is kept unless ``clear``), or None for
    make_convolutional_layer's initialisation (``sqrt(2 / (size^2 c)) * U(-1, 1)`` from numpy's generator with ``seed``:
    the distribution, not ``rand()``'s bits).  Parameters, update buffers and rolling statistics are tensors on
    ``device``, or numpy arrays with ``device=None``."""

    def __init__(self, cfgfile, weights=None, device=None, clear=False, seed=0):
        from . import _lib
        self._L = _lib
        blocks = C.parse_cfg_text(cfgfile) if "\n" in cfgfile else C.parse_cfg(cfgfile)
        self.blocks = blocks
        self.net, self.layers = parse_layers(blocks)
        self.convs = [l for l in self.layers if l["type"] == "convolutional"]
        self.heads = [l for l in self.layers if l["type"] == "yolo"]
        self.seen = 0
        self.side = _lib.Side(device)
        self.torch, self.dev = self.side.torch, self.side.dev
        flat = None
        if weights is not None:
            _, seen, flat = W.read_darknet_weights(weights)
            self.seen = 0 if clear else seen
            parts = W.split_darknet_stream(blocks[1:], flat)    # (layer numbers, as a route counts them)
        rng = np.random.default_rng(seed)
        for n, l in enumerate(self.convs):
            K, c, s = l["out"][0], l["cin"], l["size"]
            if flat is not None:
                p = parts[n]
                init = dict(weights=p["weight"], biases=p["bn_bias"] if l["bn"] else p["bias"])
                if l["bn"]:
                    init.update(scales=p["bn_weight"], rolling_mean=p["bn_mean"], rolling_variance=p["bn_var"])
            else:
                init = dict(weights=(f32(math.sqrt(2. / (s * s * c))) * rng.uniform(-1, 1, (K, c, s, s)).astype(f32)).astype(f32),
                            biases=np.zeros(K, f32))
                if l["bn"]:
                    init.update(scales=np.ones(K, f32), rolling_mean=np.zeros(K, f32), rolling_variance=np.zeros(K, f32))
            for k, v in init.items():
                l[k] = self._put(np.ascontiguousarray(v, f32))
            l["weight_updates"], l["bias_updates"] = self._zeros((K, c, s, s)), self._zeros((K,))
            if l["bn"]:
                l["scale_updates"], l["mean"], l["variance"], l["stat"] = (self._zeros((K,)), self._zeros((K,)), self._zeros((K,)),
                                                                           self._zeros((2, K)))
        self._batch = None
        self._table()

    # ------------------------------------------------------------------------------------------- arrays on either side
    def _put(self, a):
        return self.side.put(a, f32, copy=True)      # (the net owns and updates its parameters)

    def _zeros(self, shape):
        return self.side.zeros(tuple(shape), f32)

    def _get(self, a):
        return self.side.get(a, copy=True)

    def _call(self, name, *args):
        """the host twin, or the device function on the current stream"""
        self.side.call(name, *args)

    def _table(self):
        """the update's table: (parameter, update, count, kind) per tensor, on the side that runs it"""
        rows = []
        for l in self.convs:
            rows.append((l["biases"], l["bias_updates"], 0))
            if l["bn"]:
                rows.append((l["scales"], l["scale_updates"], 0))
            rows.append((l["weights"], l["weight_updates"], 1))
        ptr = (lambda a: a.ctypes.data) if self.dev is None else (lambda a: a.data_ptr())
        size = (lambda a: a.size) if self.dev is None else (lambda a: a.numel())
        t = np.array([(ptr(p), ptr(u), size(p), kind) for p, u, kind in rows], np.int64)
        chunk = int(self._L.lib().bp_train_update_chunk())
        self._blocks = int(sum((int(n) + chunk - 1) // chunk for n in t[:, 2]))
        self._tab = t if self.dev is None else self.torch.from_numpy(t).to(self.dev)
        self._ntab = len(rows)

    def _alloc(self, N):
        if self._batch == N:
            return
        self._batch = N
        for l in self.layers:
            shape = (N,) + l["out"]
            if l["type"] != "yolo":
                l["output"] = self._zeros(shape)
            l["delta"] = self._zeros(shape)
            if l["type"] == "convolutional":
                l["x"] = self._zeros(shape)
                if l["bn"]:
                    l["x_norm"] = self._zeros(shape)
                c, h, w = l["inp"]
                n = int(self._L.lib().bp_train_conv_scratch(N, c, h, w, l["out"][0], l["size"], l["stride"]))
                l["scratch"] = self._zeros((max(n, 1),))

    # ------------------------------------------------------------------------------------------- the three passes
    def _conv(self, role, l, x, w, y):
        c, h, wd = l["inp"]
        self._call("bp_train_conv", role, x, w, y, self._batch, c, h, wd, l["out"][0], l["size"], l["stride"], l["scratch"])

    def forward(self, inps, train=True):
        """forward_network: ``inps`` [B, 3, H, W] float32 as yolo_inputs makes them (an array, or a tensor on the
        device); the raw output of the convolution before each [yolo] layer, in order, as yolo_loss takes them.
        ``train`` uses and records the batch statistics and updates the rolling ones."""
        if self.dev is None:
            x = np.ascontiguousarray(np.asarray(inps), f32)
        else:
            x = (inps if hasattr(inps, "data_ptr") else self.torch.from_numpy(np.ascontiguousarray(inps, f32)))
            x = x.to(self.dev, self.torch.float32).contiguous()
        if tuple(x.shape[1:]) != (self.net["channels"], self.net["height"], self.net["width"]):
            raise ValueError("inps must be [B, %d, %d, %d]" % (self.net["channels"], self.net["height"], self.net["width"]))
        N = int(x.shape[0])
        self._alloc(N)
        self._input = x
        cat = np.concatenate if self.dev is None else self.torch.cat
        heads = []
        for i, l in enumerate(self.layers):
            t = l["type"]
            if t == "convolutional":
                K, S = l["out"][0], l["out"][1] * l["out"][2]
                self._conv(0, l, x, l["weights"], l["x"])
                self._call("bp_train_bn_forward", l["x"], N, K, S, l.get("scales"), l["biases"], l.get("rolling_mean"),
                           l.get("rolling_variance"), l.get("mean"), l.get("variance"), l.get("x_norm"), l["output"], int(l["bn"]),
                           l["leaky"], int(bool(train)))
            elif t == "shortcut":
                l["output"][...] = x + self.layers[l["src"]]["output"]
            elif t == "route":
                l["output"][...] = cat([self.layers[s]["output"] for s in l["src"]], 1)
            elif t == "upsample":
                for dy in (0, 1):
                    for dx in (0, 1):
                        l["output"][:, :, dy::2, dx::2] = x
            else:
                l["output"] = x
                heads.append(x)
            x = l["output"]
        return heads

    def backward(self, head_deltas):
        """backward_network after forward(train=True): every delta is zeroed (forward_network does that), each head's
        ``delta`` (yolo_loss's, Darknet's descent direction) enters its convolution unchanged, and every convolution's
        ``bias_updates`` / ``scale_updates`` / ``weight_updates`` are added to."""
        if len(head_deltas) != len(self.heads):
            raise ValueError("one delta per [yolo] layer")
        for l in self.layers:
            l["delta"][...] = 0
        for l, d in zip(self.heads, head_deltas):
            l["delta"][...] = d if self.dev is None or hasattr(d, "data_ptr") else self.torch.from_numpy(np.asarray(d)).to(self.dev)
        N = self._batch
        for i in range(len(self.layers) - 1, -1, -1):
            l, t = self.layers[i], self.layers[i]["type"]
            prev = self.layers[i - 1] if i else None
            if t == "convolutional":
                K, S = l["out"][0], l["out"][1] * l["out"][2]
                self._call("bp_train_bn_backward", l["output"], l["delta"], l["x"], l.get("x_norm"), l.get("mean"), l.get("variance"),
                           l.get("scales"), N, K, S, l["bias_updates"], l.get("scale_updates"), l.get("stat"), int(l["bn"]), l["leaky"])
                self._conv(1, l, prev["output"] if prev else self._input, l["weight_updates"], l["delta"])
                if prev:
                    self._conv(2, l, prev["delta"], l["weights"], l["delta"])
            elif t == "shortcut":
                prev["delta"] += l["delta"]
                self.layers[l["src"]]["delta"] += l["delta"]
            elif t == "route":
                at = 0
                for s in l["src"]:
                    c = self.layers[s]["out"][0]
                    self.layers[s]["delta"] += l["delta"][:, at:at + c]
                    at += c
            elif t == "upsample":       # upsample_cpu(forward = 0): the four adds in its loop order
                for dy in (0, 1):
                    for dx in (0, 1):
                        prev["delta"] += l["delta"][:, :, dy::2, dx::2]
            else:
                prev["delta"] += l["delta"]

    def current_rate(self):
        return learning_rate(self.net, self.seen // (self.net["batch"] * self.net["subdivisions"]))

    def update(self):
        """update_network: one launch over every parameter tensor"""
        ub = self.net["batch"] * self.net["subdivisions"]
        a, dk = f32(self.current_rate() / f32(ub)), f32(-self.net["decay"] * f32(ub))
        rates = (float(a), float(dk), float(self.net["momentum"]))
        if self.dev is None:
            self.side.call("bp_train_update", self._tab, self._ntab, *rates)
        else:
            self.side.call("bp_train_update", self._tab, self._ntab, self._blocks, *rates)

    def loss(self, heads, truth):
        """the heads' yolo_loss: (per-head deltas, per-head costs as float64 -- device tensors [1] on a device)"""
        size = (self.net["height"], self.net["width"])
        deltas, costs = [], []
        for l, x in zip(self.heads, heads):
            h = l["head"]
            if self.dev is None:
                c, _, d, _ = yolo_loss(x, truth, size, h["anchors"], h["mask"], h["classes"], h["ignore_thresh"], h["truth_thresh"],
                                       want_act=False)
            else:
                r = _loss_call(self.side, x, truth, size, h["anchors"], h["mask"], h["classes"], h["ignore_thresh"],
                               h["truth_thresh"], 0, False)
                c, d = r["cost"], r["delta"]
            deltas.append(d), costs.append(c)
        return deltas, costs

    def train_step(self, inps, truth):
        """train_network_datum: forward, the heads' loss, backward, and the update when ``seen / batch`` is a multiple
        of ``subdivisions``.  Returns get_network_cost, the float32 mean of the heads' costs: the one value read back."""
        if int(inps.shape[0]) != self.net["batch"]:
            raise ValueError("the cfg's batch / subdivisions is %d images" % self.net["batch"])
        self.seen += self.net["batch"]
        heads = self.forward(inps, train=True)
        deltas, costs = self.loss(heads, truth)
        self.last_deltas = deltas
        self.backward(deltas)
        if (self.seen // self.net["batch"]) % self.net["subdivisions"] == 0:
            self.update()
        if self.dev is not None:
            costs = self.torch.cat(costs).cpu().tolist()
        total = f32(0)
        for c in costs:
            total = f32(total + f32(c))
        return float(f32(total / f32(len(costs))))

    # ------------------------------------------------------------------------------------------- state, files
    def state(self):
        """numpy copies of every parameter, rolling statistic and update buffer: ``conv<n>.<name>``"""
        out = {}
        for n, l in enumerate(self.convs):
            for k in _PARAMS + _UPDATES:
                if k in l:
                    out["conv%d.%s" % (n, k)] = self._get(l[k])
        return out

    def load_state(self, state):
        for n, l in enumerate(self.convs):
            for k in _PARAMS + _UPDATES:
                if k in l and "conv%d.%s" % (n, k) in state:
                    v = np.ascontiguousarray(state["conv%d.%s" % (n, k)], f32).reshape(tuple(l[k].shape))
                    l[k][...] = v if self.dev is None else self.torch.from_numpy(v).to(self.dev)

    def save_weights(self, path):
        """save_weights_upto (parser.c:962): the (0, 1, 0) header with ``seen`` as an int, then per convolution biases,
        scales, rolling mean, rolling variance (batch-normalised layers) and weights."""
        flat = np.concatenate([self._get(l[k]).reshape(-1) for l in self.convs for k in _PARAMS if k in l])
        W.write_darknet_weights(path, flat, seen=self.seen, version=(0, 1, 0))
