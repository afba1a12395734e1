"""What the training-iteration tests share (test_darknet_train_host.py, test_gpu_darknet_train.py): the golden archive with
its meta, the tiny nets built from it, the bar helper and the per-kernel shapes."""
import functools
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_BOXES = 90
FLOOR = 2.0 ** -23


@functools.lru_cache(maxsize=None)
def golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "darknet_train.npz"))
    out = {k: g[k] for k in g.files}
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def meta():
    return json.loads(bytes(golden()["meta"]).decode())


def bar(q):
    """the bar of quantity ``q``: max(4 * ref_err[q], 2^-23), from the archive"""
    return max(4.0 * meta()["ref_err"][q], FLOOR)


def distance(ours, ref):
    """max|ours - ref| / max|ref| (0 for two all-zero tensors)"""
    ours, ref = np.asarray(ours, np.float64), np.asarray(ref, np.float64)
    assert ours.shape == ref.shape, (ours.shape, ref.shape)
    m = float(np.abs(ref).max())
    d = float(np.abs(ours - ref).max())
    return d / m if m > 0 else d


def check(q, ours, name=None, out=None):
    """assert quantity ``q`` of the archive within its bar; prints the figure first"""
    d, b = distance(ours, golden()[q]), bar(q)
    print("%-44s %.3e  bar %.3e" % (q, d, b))
    assert d <= b, (q, d, b)


def case_batch(name, k):
    """(inps, truth [B, 90, 5]) of call ``k`` of case ``name`` (a case with one fixed batch has only call 0's)"""
    g, c = golden(), meta()["cases"][name]
    k = 0 if c["fixed_batch"] else k
    t = np.zeros((c["batch"], MAX_BOXES, 5), np.float32)
    kept = np.array(g["%s.%d.truth" % (name, k)])
    t[:, :kept.shape[1]] = kept
    return np.array(g["%s.%d.inps" % (name, k)]), t


def initial_state(name):
    g = golden()
    p = name + ".init."
    return {k[len(p):]: np.array(v) for k, v in g.items() if k.startswith(p)}


def make_net(name, device=None):
    """the tiny net of case ``name`` with the archive's initial parameters"""
    from betapose_amd.darknet_train import TrainableDarknet
    net = TrainableDarknet(meta()["cases"][name]["cfg"], device=device)
    net.load_state(initial_state(name))
    return net


def state_of(name, k):
    """the reference's parameters, rolling statistics and update buffers after call ``k``"""
    g = golden()
    p = "%s.%d.post." % (name, k)
    return {q[len(p):]: np.array(v) for q, v in g.items() if q.startswith(p)}


def group_a_step(net, name):
    """One step of a group A case in its parts: (every quantity the archive holds a bar for, the heads' own deltas).
    The bars of the backward pass were formed with the reference's own yolo deltas going in, so they go in here too."""
    g = golden()
    as_np = lambda a: np.array(a) if isinstance(a, np.ndarray) else a.cpu().numpy()
    inps, truth = case_batch(name, 0)
    net.seen += net.net["batch"]
    heads = net.forward(inps, train=True)
    q = {}
    for n, l in enumerate(net.convs):
        q["%s.0.fwd.conv%d.output" % (name, n)] = as_np(l["output"])
        if l["bn"]:
            q["%s.0.fwd.conv%d.mean" % (name, n)], q["%s.0.fwd.conv%d.variance" % (name, n)] = as_np(l["mean"]), as_np(l["variance"])
    deltas, costs = net.loss(heads, truth)
    costs = [np.float32(c if isinstance(c, float) else c.cpu().numpy()[0]) for c in costs]
    q["%s.0.cost" % name] = np.float32(np.mean(costs, dtype=np.float32))
    net.backward([np.array(g["%s.0.yolo%d.delta" % (name, h)]) for h in range(len(deltas))])
    for k, v in net.state().items():
        if k.endswith("_updates"):
            q["%s.0.pre.%s" % (name, k)] = v
    net.update()
    for k, v in net.state().items():
        q["%s.0.post.%s" % (name, k)] = v
    return q, [as_np(d) for d in deltas]


# ---------------------------------------------------------------------------------------------------- kernels alone
# name, N, Cin, H, W, Cout, size, stride: neither channel count a multiple of a tile, 1 x 1 and 3 x 3, stride 2 on odd
# sizes, a 2 x 2 map, K = 720 (several k steps and a partial last one), N 1 and 3, a filter gradient over more than one
# reduction slice (3 * 26 * 26 = 2028 < 2048 < 3 * 27 * 27) and one that does not fill the first
CONV_SHAPES = [("c3_k18_3x3", 3, 3, 9, 11, 18, 3, 1), ("c3_k18_1x1", 1, 3, 6, 5, 18, 1, 1), ("s2_13", 1, 5, 13, 13, 7, 3, 2),
               ("s2_5x7", 3, 4, 5, 7, 6, 3, 2), ("map2x2", 3, 6, 2, 2, 5, 3, 1), ("c80", 1, 80, 4, 5, 18, 3, 1),
               ("s2_1x1", 1, 9, 7, 6, 4, 1, 2), ("slices", 3, 3, 27, 27, 18, 3, 1), ("wide", 1, 3, 8, 9, 70, 1, 1)]


def conv_case(shape, seed=7):
    """(x, w, delta of the output, a non-zero delta of the input, non-zero filter updates) of one shape"""
    _, N, C, H, W, K, size, stride = shape
    rng = np.random.default_rng([seed, N, C, H, W, K, size, stride])
    pad = size // 2
    OH, OW = (H + 2 * pad - size) // stride + 1, (W + 2 * pad - size) // stride + 1
    f = lambda *s: rng.normal(0, 1, s).astype(np.float32)
    return f(N, C, H, W), f(K, C, size, size), f(N, K, OH, OW), f(N, C, H, W), f(K, C, size, size)


def conv_reference(role, x, w, dy, dx0, wu0, stride):
    """the same GEMM in float64, summed any way: (y, filter updates, input delta)"""
    x, w, dy = x.astype(np.float64), w.astype(np.float64), dy.astype(np.float64)
    N, C, H, W = x.shape
    K, _, s, _ = w.shape
    p = s // 2
    OH, OW = dy.shape[2:]
    xp = np.pad(x, ((0, 0), (0, 0), (p, p), (p, p)))
    cols = np.stack([xp[:, :, ky:ky + stride * OH:stride, kx:kx + stride * OW:stride] for ky in range(s) for kx in range(s)], 2)
    if role == 0:
        return np.einsum("nctyx,kct->nkyx", cols, w.reshape(K, C, s * s))
    if role == 1:
        return wu0 + np.einsum("nkyx,nctyx->kct", dy, cols).reshape(w.shape)
    dc = np.einsum("nkyx,kct->nctyx", dy, w.reshape(K, C, s * s))
    buf = np.zeros_like(xp)
    for ky in range(s):
        for kx in range(s):
            buf[:, :, ky:ky + stride * OH:stride, kx:kx + stride * OW:stride] += dc[:, :, ky * s + kx]
    return dx0 + buf[:, :, p:p + H, p:p + W]


def run_conv(role, shape, x, w, y, device=None, stream=None):
    """bp_train_conv(_host) in place on arrays (device None) or tensors: role 0 writes y, 1 adds to w, 2 adds to x"""
    from betapose_amd import _lib
    _, N, C, H, W, K, size, stride = shape
    n = max(int(_lib.lib().bp_train_conv_scratch(N, C, H, W, K, size, stride)), 1)
    if device is None:
        scratch = np.full(n, np.nan, np.float32)
        _lib.check(_lib.lib().bp_train_conv_host(role, _lib.ptr(x), _lib.ptr(w), _lib.ptr(y), N, C, H, W, K, size, stride,
                                                 _lib.ptr(scratch)))
    else:
        import torch
        scratch = torch.full((n,), float("nan"), device=device)
        _lib.check(_lib.lib().bp_train_conv(role, _lib.ptr(x), _lib.ptr(w), _lib.ptr(y), N, C, H, W, K, size, stride, _lib.ptr(scratch),
                                            stream if stream is not None else torch.cuda.current_stream().cuda_stream))


BN_SHAPES = [(1, 10, 4), (3, 10, 169), (3, 70, 4), (1, 70, 169)]      # N, C, S


def bn_case(N, C, S, seed=3):
    rng = np.random.default_rng([seed, N, C, S])
    f = lambda *s: rng.normal(0, 1, s).astype(np.float32)
    return dict(x=f(N, C, S) * 2 + 0.5, scales=rng.uniform(.5, 1.5, C).astype(np.float32), biases=f(C), rolling_mean=f(C),
                rolling_var=rng.uniform(.5, 1.5, C).astype(np.float32), delta=f(N, C, S), bias_updates=f(C), scale_updates=f(C))


def run_bn(c, N, C, S, bn, leaky, device=None, stream=None):
    """forward (train) then backward of one layer on copies of case ``c``: a dict of every tensor written"""
    from betapose_amd import _lib
    L = _lib.lib()
    if device is None:
        put = lambda a: np.array(a)
        new = lambda *s: np.full(s, np.nan, np.float32)
        tail, sfx = (), "_host"
    else:
        import torch
        put = lambda a: torch.from_numpy(np.array(a)).to(device)
        new = lambda *s: torch.full(s, float("nan"), device=device)
        tail, sfx = (stream if stream is not None else torch.cuda.current_stream().cuda_stream,), ""
    t = {k: put(v) for k, v in c.items()}
    t.update(mean=new(C), var=new(C), x_norm=new(N, C, S), out=new(N, C, S), stat=new(2, C))
    p = _lib.ptr
    _lib.check(getattr(L, "bp_train_bn_forward" + sfx)(p(t["x"]), N, C, S, p(t["scales"]), p(t["biases"]), p(t["rolling_mean"]),
                                                       p(t["rolling_var"]), p(t["mean"]), p(t["var"]), p(t["x_norm"]), p(t["out"]),
                                                       bn, leaky, 1, *tail))
    _lib.check(getattr(L, "bp_train_bn_backward" + sfx)(p(t["out"]), p(t["delta"]), p(t["x"]), p(t["x_norm"]), p(t["mean"]),
                                                        p(t["var"]), p(t["scales"]), N, C, S, p(t["bias_updates"]),
                                                        p(t["scale_updates"]), p(t["stat"]), bn, leaky, *tail))
    keys = ["out", "delta", "bias_updates"] + (["mean", "var", "x_norm", "rolling_mean", "rolling_var", "scale_updates", "stat"] if bn else [])
    return {k: (t[k] if device is None else t[k].cpu().numpy()) for k in keys}


UPDATE_COUNTS = (1, 3, 64, 1000, 4099)


def update_case(seed=5):
    rng = np.random.default_rng(seed)
    return [(rng.normal(0, 1, n).astype(np.float32), rng.normal(0, 1, n).astype(np.float32), i % 2) for i, n in enumerate(UPDATE_COUNTS)]


def update_reference(rows, a, dk, mom):
    """three separate float32 axpy / scal passes in numpy"""
    out = []
    a, dk, mom = np.float32(a), np.float32(dk), np.float32(mom)
    for p, u, kind in rows:
        p, u = p.copy(), u.copy()
        if kind:
            u = (u + (dk * p).astype(np.float32)).astype(np.float32)
        p = (p + (a * u).astype(np.float32)).astype(np.float32)
        u = (u * mom).astype(np.float32)
        out.append((p, u))
    return out
