"""What the key-point-detector training tests share (test_kpd_train_host.py, test_gpu_kpd_train.py): the golden archive
with its meta and bars, the tiny net built from it, one caller for a kernel on either side, the per-kernel shapes and
cases, and a torch mirror of the module list built from weights.fastpose_modules() with torch.nn.functional."""
import functools
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 2.0 ** -23
f32 = np.float32

# (N, C, S): N * S = 2; S not a multiple of 4; N * S just over 256 and just over 1 024; C = 1
BN_SHAPES = [(2, 3, 1), (1, 2, 2), (3, 5, 7), (1, 1, 260), (2, 3, 129), (4, 2, 260), (257, 2, 4), (1, 1, 1028), (3, 4, 343)]
POOL_S = [1, 6, 5120]
MAXPOOL_SHAPES = [(3, 18, 14), (2, 5, 5), (2, 1, 9), (1, 4, 1)]
# (name, N, C, H, W, K, size, stride)
CONV7_SHAPES = [("9x11", 2, 3, 9, 11, 5, 7, 2), ("14x10", 1, 3, 14, 10, 4, 7, 2)]
LINEAR_SHAPES = [("b1", 1, 8, 1, 1, 8, 1, 1), ("b3", 3, 8, 1, 1, 8, 1, 1)]
RMSPROP_COUNTS = (1, 1023, 1025, 1030)      # the last row is misaligned on the device
RMSPROP_SETTINGS = [dict(lr=1e-3, alpha=0.99, eps=1e-8, wd=0.0, momentum=0.0), dict(lr=1e-3, alpha=0.99, eps=1e-8, wd=1e-4, momentum=0.9),
                    dict(lr=1e-2, alpha=0.99, eps=1e-8, wd=1e-4, momentum=0.0), dict(lr=1e-2, alpha=0.99, eps=1e-8, wd=0.0, momentum=0.9)]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


# ------------------------------------------------------------------------------------------------ the archive
@functools.lru_cache(maxsize=None)
def golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "kpd_train.npz"))
    out = {k: g[k] for k in g.files}
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def meta():
    return json.loads(bytes(golden()["meta"]).decode())


def split(vec, keys):
    """a flat vector of the archive as a dict over ``keys``"""
    out, at = {}, 0
    for k in keys:
        shape = tuple(meta()["shapes"][k])
        n = int(np.prod(shape)) if shape else 1
        out[k] = np.array(vec[at:at + n], dtype=np.float32).reshape(shape)
        at += n
    assert at == len(vec)
    return out


def distance(ours, ref):
    ours, ref = np.asarray(ours, np.float64), np.asarray(ref, np.float64)
    assert ours.shape == ref.shape, (ours.shape, ref.shape)
    m, d = float(np.abs(ref).max()), float(np.abs(ours - ref).max())
    return d / m if m > 0 else d


def check(q, ours, ref=None, err=None):
    """assert quantity ``q`` within max(4 * ref_err[q], 2^-23) of the archive's value; prints the figure first"""
    g = golden()
    d = distance(ours, g[q] if ref is None else ref)
    b = max(4.0 * float(g["err." + q] if err is None else err), FLOOR)
    print("%-40s %.3e  bar %.3e" % (q, d, b))
    assert d <= b, (q, d, b)


SMALL = 4       # a tensor of at most this many values: see ref_err()


@functools.lru_cache(maxsize=None)
def ref_err(kind, key):
    """The archive's ref_err of tensor ``key`` for every recorded iteration that has quantity ``kind`` ('grad', 'P', 'V',
    'B'): {tag: ref_err}.  One per tensor and iteration, as the generator measured it."""
    g, m = golden(), meta()
    keys = m["keys"] if kind == "P" else m["param_keys"]
    at = keys.index(key)
    return {k[4:-len(kind) - 1]: float(v[at]) for k, v in g.items() if k.startswith("err.s") and k.endswith("." + kind)}


def tensor_bar(kind, tag, key):
    """max(4 * ref_err, 2^-23) with the tensor's OWN ref_err of this iteration.  The one exception, for a tensor of at
    most SMALL values (the batch-norm parameters of the two-channel layers, conv_out's bias): its ref_err is the maximum
    of two to four error samples, which for a cancelling sum can fall far below the error's scale by chance (recorded:
    1.0e-6 in one iteration, 1.9e-5 in another, for the same two-value tensor), so a single draw does not say what a
    second float32 evaluation may differ by.  Such a tensor takes the worst of its own ref_err over the recorded
    iterations: five independent draws of the same tensor's error, still per tensor and still the reference's alone."""
    own = ref_err(kind, key)
    shape = meta()["shapes"][key]
    small = (int(np.prod(shape)) if shape else 1) <= SMALL
    return max(4.0 * (max(own.values()) if small else own[tag]), FLOOR)


def check_vector(q, ours, keys, sub=None):
    """a per-parameter quantity of one iteration (a dict over ``keys``) against the archive's flat vector: each tensor's
    distance, normalised by that tensor's own maximum, against that tensor's own bar (tensor_bar).  ``sub`` restricts
    the check to some of the keys (the parameters, or the running statistics, of a state vector)."""
    tag, kind = q.rsplit(".", 1)
    ref = split(golden()[q], keys)
    worst = 0.0
    for k in keys:
        if sub is not None and k not in sub:
            continue
        d, b = distance(ours[k], ref[k]), tensor_bar(kind, tag, k)
        worst = max(worst, d / b)
        assert d <= b, (q, k, d, b)
    print("%-40s worst distance / bar %.3f" % (q, worst))


def batch(i):
    g = golden()
    return (g["batch%d.inps_q" % i].astype(f32) / f32(32), g["batch%d.labels_q" % i].astype(f32) / f32(255), g["batch%d.mask" % i].astype(f32))


def make_net(setting=0, device=None, **kw):
    from betapose_amd.kpd_train import TrainableFastPose
    m = meta()
    return TrainableFastPose(m["n_classes"], m["stages"], m["stem"], device=device, flip_pairs=m["flip_pairs"], **dict(m["settings"][setting], **kw))


def state_before(setting, it):
    """(state dict, optimiser state) recorded before iteration ``it``: the initial state, or the state after ``it - 1``"""
    g, m = golden(), meta()
    keys, pk = m["keys"], m["param_keys"]
    if it == 0:
        P = split(g["init.P"], keys)
        zero = {k: np.zeros_like(P[k]) for k in pk}
        return P, dict(step=0, **{"square_avg/" + k: zero[k] for k in pk}, **{"momentum_buffer/" + k: zero[k] for k in pk})
    return state_after(setting, it - 1)


def state_after(setting, it):
    g, m = golden(), meta()
    tag = "s%d.i%d" % (setting, it)
    P, V = split(g[tag + ".P"], m["keys"]), split(g[tag + ".V"], m["param_keys"])
    Bf = split(g[tag + ".B"], m["param_keys"]) if tag + ".B" in g else {k: np.zeros_like(v) for k, v in V.items()}
    return P, dict(step=it + 1, **{"square_avg/" + k: V[k] for k in V}, **{"momentum_buffer/" + k: Bf[k] for k in Bf})


def load(net, setting, it):
    P, O = state_before(setting, it)
    net.load_state_dict(P)
    net.load_optimizer_state(O)


def teacher_forced(net, setting, it):
    """one recorded iteration from its recorded state: a dict of every quantity the archive holds for it.  The forward
    and backward pass run on the net's own gradients; the update is then fed the reference's recorded gradients."""
    g, m = golden(), meta()
    tag = "s%d.i%d" % (setting, it)
    load(net, setting, it)
    inps, labels, mask = batch(it)
    before = dict(net.nbt)
    out = net.forward(inps, train=True)
    q = {"out": net._get(out)}
    loss, acc, grad = net._loss(out, labels, mask, True)
    net.zero_grad()
    net.backward(grad)
    q["loss"], q["acc"] = net._read(loss, acc)
    q["grad"] = net.grads()
    sd = {k: v.numpy() for k, v in net.state_dict().items()}
    q["running"] = {k: sd[k] for k in m["keys"] if k not in m["param_keys"]}
    q["num_batches_tracked"] = {k: int(sd[k + ".num_batches_tracked"]) - before[k] for k in before}
    net.load_grads(split(g[tag + ".grad"], m["param_keys"]))
    net.update()
    q["P"] = {k: v.numpy() for k, v in net.state_dict().items() if k in m["param_keys"]}
    o = net.optimizer_state()
    q["V"] = {k: o["square_avg/" + k] for k in m["param_keys"]}
    q["B"] = {k: o["momentum_buffer/" + k] for k in m["param_keys"]}
    return q


def check_teacher_forced(q, setting, it):
    g, m = golden(), meta()
    tag = "s%d.i%d" % (setting, it)
    pk = m["param_keys"]
    check(tag + ".out", q["out"])
    check(tag + ".loss", q["loss"])
    assert f32(q["acc"]) == f32(g[tag + ".acc"]), (q["acc"], g[tag + ".acc"])
    check_vector(tag + ".grad", q["grad"], pk)
    running = [k for k in m["keys"] if k not in pk]
    check_vector(tag + ".P", q["running"], m["keys"], running)
    check_vector(tag + ".P", q["P"], m["keys"], pk)
    check_vector(tag + ".V", q["V"], pk)
    if tag + ".B" in g:
        check_vector(tag + ".B", q["B"], pk)
    assert set(q["num_batches_tracked"].values()) == {1}      # every batch norm counted this one forward pass


def same_bits(a, b, what=""):
    """two results of teacher_forced / validate equal bit for bit"""
    if isinstance(a, dict):
        assert a.keys() == b.keys()
        for k in a:
            same_bits(a[k], b[k], "%s/%s" % (what, k))
    elif isinstance(a, (float, int)):
        assert a == b, (what, a, b)
    else:
        assert np.array_equal(bits(a), bits(b)), (what, float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max()))


def validate(net):
    """the recorded valid() batch from the state after setting 0: (loss, acc, maps)"""
    m = meta()
    P, _ = state_after(0, m["iters"] - 1)
    net.load_state_dict(P)
    inps, labels, mask = batch(m["iters"])
    loss, acc, maps = net.validate_step(inps, labels, mask, return_maps=True)
    return loss, acc, net._get(maps)


def check_validate(r):
    g = golden()
    check("valid.loss", r[0])
    assert f32(r[1]) == f32(g["valid.acc"]), (r[1], g["valid.acc"])
    check("valid.maps", r[2])


def free_run(net, steps=20):
    """``steps`` iterations of train_step over the three recorded batches in turn, from the initial state"""
    load(net, 0, 0)
    return [net.train_step(*batch(k % meta()["iters"])) for k in range(steps)]


# ------------------------------------------------------------------------------------------------ one kernel, either side
def kcall(name, args, dev=None, stream=None):
    """``bp_<name>`` on numpy arrays: the host twin, or (with ``dev``) the device function on copies of the arrays, which
    are copied back into them afterwards.  The same array passed twice is the same tensor on the device."""
    from betapose_amd import _lib
    L = _lib.lib()
    if dev is None:
        _lib.check(getattr(L, "bp_" + name + "_host")(*[_lib.ptr(a) if (a is None or hasattr(a, "shape")) else a for a in args]))
        return
    import torch
    t = {}
    for a in args:
        if hasattr(a, "shape") and id(a) not in t:
            t[id(a)] = torch.from_numpy(a).to(dev)
    s = torch.cuda.current_stream() if stream is None else stream
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _lib.check(getattr(L, "bp_" + name)(*[t[id(a)].data_ptr() if hasattr(a, "shape") else a for a in args], s.cuda_stream))
    s.synchronize()
    for a in args:
        if hasattr(a, "shape"):
            a[...] = t[id(a)].cpu().numpy()


def bn_case(N, C, S, seed=0):
    r = np.random.default_rng([seed, N, C, S])
    return dict(x=r.standard_normal((N, C, S)).astype(f32) * f32(1.5) + r.standard_normal((1, C, 1)).astype(f32),
                w=r.uniform(0.5, 1.5, C).astype(f32), b=r.standard_normal(C).astype(f32), rm=r.standard_normal(C).astype(f32),
                rv=r.uniform(0.5, 2, C).astype(f32), dy=r.standard_normal((N, C, S)).astype(f32))


def run_bn(c, N, C, S, bn, relu, train=1, dev=None, stream=None):
    """forward then backward of one case: every output, as a dict"""
    nan = lambda *shape: np.full(shape, np.nan, f32)
    o = dict(rm=c["rm"].copy(), rv=c["rv"].copy(), mean=nan(C), invstd=nan(C), out=nan(N, C, S), d=c["dy"].copy(),
             gw=np.full(C, 0.25, f32), gb=np.full(C, -0.5, f32))
    x, w = c["x"].copy(), c["w"].copy()
    kcall("kpd_train_bn_forward", [x, N, C, S, w if bn else None, c["b"].copy(), o["rm"] if bn else None, o["rv"] if bn else None,
                                   o["mean"] if bn else None, o["invstd"] if bn else None, o["out"], bn, relu, train], dev, stream)
    if train:
        kcall("kpd_train_bn_backward", [o["out"], o["d"], x if bn else None, o["mean"] if bn else None, o["invstd"] if bn else None,
                                        w if bn else None, N, C, S, o["gw"] if bn else None, o["gb"], bn, relu], dev, stream)
    return o


def tail_case(N, C, S, seed=1):
    r = np.random.default_rng([seed, N, C, S])
    return dict(y=r.standard_normal((N, C, S)).astype(f32), s=r.uniform(0.1, 0.9, (N, C)).astype(f32),
                res=r.standard_normal((N, C, S)).astype(f32), dout=r.standard_normal((N, C, S)).astype(f32),
                dres=r.standard_normal((N, C, S)).astype(f32))


def run_tail(c, N, C, S, gate, dev=None, stream=None):
    o = dict(out=np.full((N, C, S), np.nan, f32), dres=c["dres"].copy(), dy=np.full((N, C, S), np.nan, f32), ds=np.full((N, C), np.nan, f32))
    s = c["s"].copy() if gate else None
    kcall("kpd_train_tail_forward", [c["y"].copy(), s, c["res"].copy(), o["out"], N, C, S], dev, stream)
    kcall("kpd_train_tail_backward", [o["out"], c["dout"].copy(), c["y"].copy(), s, o["dres"], o["dy"], o["ds"] if gate else None, N, C, S],
          dev, stream)
    if not gate:
        o.pop("ds")
    return o


def run_pool(y, dpool, dy0, dev=None, stream=None):
    rows, S = y.shape
    o = dict(pool=np.full(rows, np.nan, f32), dy=dy0.copy())
    kcall("kpd_train_pool_forward", [y.copy(), rows, S, o["pool"]], dev, stream)
    kcall("kpd_train_pool_backward", [dpool.copy(), o["dy"], rows, S], dev, stream)
    return o


def run_sigmoid(x, g, dev=None, stream=None):
    o = dict(s=np.full(x.shape, np.nan, f32), g=g.copy())
    kcall("kpd_train_sigmoid_forward", [x.copy(), o["s"], x.size], dev, stream)
    kcall("kpd_train_sigmoid_backward", [o["s"], o["g"], x.size], dev, stream)
    return o


def run_maxpool(x, dout, dev=None, stream=None):
    P, H, W = x.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    o = dict(out=np.full((P, OH, OW), np.nan, f32), arg=np.full((P, OH, OW), -7, np.int32), dx=np.full((P, H, W), np.nan, f32))
    kcall("kpd_train_maxpool_forward", [x.copy(), P, H, W, o["out"], o["arg"]], dev, stream)
    kcall("kpd_train_maxpool_backward", [dout.copy(), o["arg"], P, H, W, o["dx"]], dev, stream)
    return o


def conv_case(shape, seed=2):
    _, N, C, H, W, K, size, stride = shape
    r = np.random.default_rng([seed, N, C, H, W, K])
    OH, OW = (H + 2 * (size // 2) - size) // stride + 1, (W + 2 * (size // 2) - size) // stride + 1
    return dict(x=r.standard_normal((N, C, H, W)).astype(f32), w=r.standard_normal((K, C, size, size)).astype(f32),
                dy=r.standard_normal((N, K, OH, OW)).astype(f32), dx0=r.standard_normal((N, C, H, W)).astype(f32),
                dw0=r.standard_normal((K, C, size, size)).astype(f32))


def run_conv(c, shape, dev=None, stream=None):
    """the three roles: y, dw (added to dw0), dx (added to dx0)"""
    from betapose_amd import _lib
    _, N, C, H, W, K, size, stride = shape
    geom = [N, C, H, W, K, size, stride]
    scratch = np.zeros(max(int(_lib.lib().bp_kpd_train_conv_scratch(*geom)), 1), f32)
    o = dict(y=np.full(c["dy"].shape, np.nan, f32), dw=c["dw0"].copy(), dx=c["dx0"].copy())
    kcall("kpd_train_conv", [0, c["x"].copy(), c["w"].copy(), o["y"]] + geom + [scratch], dev, stream)
    kcall("kpd_train_conv", [1, c["x"].copy(), o["dw"], c["dy"].copy()] + geom + [scratch], dev, stream)
    kcall("kpd_train_conv", [2, o["dx"], c["w"].copy(), c["dy"].copy()] + geom + [scratch], dev, stream)
    return o


def rmsprop_case(seed=3):
    r = np.random.default_rng(seed)
    rows = []
    for n in RMSPROP_COUNTS:
        g = r.standard_normal(n).astype(f32)
        g[0] = 0        # a zero-gradient element: sqrt(v) + eps keeps the quotient finite
        rows.append(dict(p=r.standard_normal(n).astype(f32), g=g, v=(r.uniform(0, 1, n) ** 2).astype(f32), b=r.standard_normal(n).astype(f32) * f32(0.1)))
    rows[0]["v"][0] = 0
    return rows


def run_rmsprop(rows, h, dev=None, stream=None):
    """one step over copies of ``rows``: a list of dicts p, v, b"""
    from betapose_amd import _lib
    out = [{k: v.copy() for k, v in row.items()} for row in rows]
    hp = [h["lr"], h["alpha"], h["eps"], h["wd"], h["momentum"]]
    if dev is None:
        table = np.array([(o["p"].ctypes.data, o["g"].ctypes.data, o["v"].ctypes.data, o["b"].ctypes.data, o["p"].size) for o in out], np.int64)
        _lib.check(_lib.lib().bp_kpd_train_rmsprop_host(table.ctypes.data, len(out), *hp))
        return out
    import torch
    def put(v, shift):          # (shift: a view one float into a longer buffer, so the row is not 16-byte aligned)
        if not shift:
            return torch.from_numpy(v).to(dev)
        buf = torch.zeros(v.size + 1, dtype=torch.float32, device=dev)
        buf[1:] = torch.from_numpy(v).to(dev)
        return buf[1:]
    t = [{k: put(v, i == len(out) - 1) for k, v in o.items()} for i, o in enumerate(out)]
    table = torch.tensor([(o["p"].data_ptr(), o["g"].data_ptr(), o["v"].data_ptr(), o["b"].data_ptr(), o["p"].numel()) for o in t],
                         dtype=torch.int64, device=dev)
    chunk = int(_lib.lib().bp_kpd_train_update_chunk())
    blocks = sum((o["p"].size + chunk - 1) // chunk for o in out)
    s = torch.cuda.current_stream() if stream is None else stream
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _lib.check(_lib.lib().bp_kpd_train_rmsprop(table.data_ptr(), len(t), blocks, *hp, s.cuda_stream))
    s.synchronize()
    return [{k: v.cpu().numpy() for k, v in o.items()} for o in t]


# ------------------------------------------------------------------------------------------------ the torch mirror
def mirror_forward(P, x, stages, train):
    """FastPose_SE's forward over a dict of tensors keyed as the state dict, from weights.fastpose_modules()' names, with
    torch.nn.functional.  Running statistics are read, never written."""
    import torch
    F = torch.nn.functional

    def bn(name, y):
        return F.batch_norm(y, None if train else P[name + ".running_mean"], None if train else P[name + ".running_var"],
                            P[name + ".weight"], P[name + ".bias"], training=train, momentum=0.1, eps=1e-5)

    y = F.max_pool2d(F.relu(bn("preact.bn1", F.conv2d(x, P["preact.conv1.weight"], stride=2, padding=3))), 3, 2, 1)
    for li, (planes, nblocks, stride) in enumerate(stages, start=1):
        for bi in range(nblocks):
            pre, s = "preact.layer%d.%d" % (li, bi), (stride if bi == 0 else 1)
            o = F.relu(bn(pre + ".bn1", F.conv2d(y, P[pre + ".conv1.weight"])))
            o = F.relu(bn(pre + ".bn2", F.conv2d(o, P[pre + ".conv2.weight"], stride=s, padding=1)))
            o = bn(pre + ".bn3", F.conv2d(o, P[pre + ".conv3.weight"]))
            if pre + ".se.fc.0.weight" in P:
                g = F.relu(F.linear(o.mean((2, 3)), P[pre + ".se.fc.0.weight"], P[pre + ".se.fc.0.bias"]))
                g = torch.sigmoid(F.linear(g, P[pre + ".se.fc.2.weight"], P[pre + ".se.fc.2.bias"]))
                o = o * g[:, :, None, None]
                res = bn(pre + ".downsample.1", F.conv2d(y, P[pre + ".downsample.0.weight"], stride=s))
            else:
                res = y
            y = F.relu(o + res)
    y = F.pixel_shuffle(y, 2)
    for d in ("duc1", "duc2"):
        y = F.pixel_shuffle(F.relu(bn(d + ".bn", F.conv2d(y, P[d + ".conv.weight"], padding=1))), 2)
    return F.conv2d(y, P["conv_out.weight"], P["conv_out.bias"], padding=1)
