"""What the training-iteration tests share (test_darknet_train_host.py, test_gpu_darknet_train.py): the golden archive with
its meta, the tiny nets built from it, the bar helper, the per-kernel shapes, and the seeded inputs of the shipped
topology's step and of the non-square tiny net (the fixture maker calls these too)."""
import functools
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_BOXES = 90
FLOOR = 2.0 ** -23


@functools.lru_cache(maxsize=None)
def golden(archive="darknet_train"):
    g = np.load(os.path.join(ROOT, "tests", "golden", archive + ".npz"))
    out = {k: g[k] for k in g.files}
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def meta(archive="darknet_train"):
    return json.loads(bytes(golden(archive)["meta"]).decode())


def bar(q, archive="darknet_train"):
    """the bar of quantity ``q``: max(4 * ref_err[q], 2^-23), from the archive"""
    return max(4.0 * meta(archive)["ref_err"][q], FLOOR)


def distance(ours, ref):
    """max|ours - ref| / max|ref| (0 for two all-zero tensors)"""
    ours, ref = np.asarray(ours, np.float64), np.asarray(ref, np.float64)
    assert ours.shape == ref.shape, (ours.shape, ref.shape)
    m = float(np.abs(ref).max())
    d = float(np.abs(ours - ref).max())
    return d / m if m > 0 else d


def check(q, ours, against=None, bar_of=None, archive="darknet_train", quiet=False):
    """assert quantity ``q`` within its bar of the archive's record of it (or of ``against``, where the archive holds
    only the bar; ``bar_of`` names another quantity's bar); prints the figure first.  Returns distance / bar."""
    d, b = distance(ours, golden(archive)[q] if against is None else against), bar(bar_of or q, archive)
    if not quiet:
        print("%-44s %.3e  bar %.3e" % (q, d, b))
    assert d <= b, (q, d, b)
    return d / b


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


def step_in_parts(net, name, inps, truth, fed):
    """One step in its parts under the quantity names of case ``name``: every convolution's output, batch mean and
    variance, the cost, every update buffer before the update, every parameter, rolling statistic and update buffer
    after it; and the heads' own deltas.  ``fed``: the yolo deltas that enter the backward pass."""
    as_np = lambda a: np.array(a) if isinstance(a, np.ndarray) else a.cpu().numpy()
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
    net.backward([np.array(d) for d in fed])
    for k, v in net.state().items():
        if k.endswith("_updates"):
            q["%s.0.pre.%s" % (name, k)] = v
    net.update()
    for k, v in net.state().items():
        q["%s.0.post.%s" % (name, k)] = v
    return q, [as_np(d) for d in deltas]


def group_a_step(net, name):
    """One step of a group A case in its parts: (every quantity the archive holds a bar for, the heads' own deltas).
    The bars of the backward pass were formed with the reference's own yolo deltas going in, so they go in here too."""
    g = golden()
    inps, truth = case_batch(name, 0)
    return step_in_parts(net, name, inps, truth, [g["%s.0.yolo%d.delta" % (name, h)] for h in range(len(net.heads))])


# ---------------------------------------------------------------------------------------------------- the tiny net
ANCHORS = [(2, 3), (4, 3), (3, 5), (6, 8), (10, 7), (12, 13)]


def tiny_cfg(width, height, batch, subdivisions, classes, net_extra):
    A = 3 * (5 + classes)

    def conv(filters, size, stride, bn=True, act="leaky"):
        return ("[convolutional]\n" + ("batch_normalize=1\n" if bn else "") +
                "filters=%d\nsize=%d\nstride=%d\npad=1\nactivation=%s\n\n" % (filters, size, stride, act))

    def yolo(mask):
        return ("[yolo]\nmask = %s\nanchors = %s\nclasses=%d\nnum=%d\njitter=.3\nignore_thresh = .7\ntruth_thresh = 1\nrandom=0\n\n"
                % (",".join(str(m) for m in mask), ",  ".join("%d,%d" % a for a in ANCHORS), classes, len(ANCHORS)))
    return ("[net]\nbatch=%d\nsubdivisions=%d\nwidth=%d\nheight=%d\nchannels=3\nmomentum=0.9\ndecay=0.0005\n%s\n"
            % (batch, subdivisions, width, height, net_extra) +
            conv(6, 3, 1) + conv(10, 3, 2) + conv(5, 1, 1) + conv(10, 3, 1) + "[shortcut]\nfrom=-3\nactivation=linear\n\n" +
            conv(12, 3, 2) + conv(A, 1, 1, False, "linear") + yolo((3, 4, 5)) + "[route]\nlayers = -4\n\n" + conv(6, 1, 1) +
            "[upsample]\nstride=2\n\n" + "[route]\nlayers = -1, 0\n\n" + conv(8, 3, 1) + conv(A, 1, 1, False, "linear") + yolo((0, 1, 2)))


EPS_ZERO, EPS_IOU, EPS_ANCHOR, EPS_CELL = 1e-5, 1e-4, 1e-6, 1e-4


def iou64(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)

    def ov(x1, w1, x2, w2):
        return np.minimum(x1 + w1 / 2, x2 + w2 / 2) - np.maximum(x1 - w1 / 2, x2 - w2 / 2)
    w, h = ov(a[..., 0], a[..., 2], b[..., 0], b[..., 2]), ov(a[..., 1], a[..., 3], b[..., 1], b[..., 3])
    inter = np.where((w < 0) | (h < 0), 0.0, w * h)
    return inter / (a[..., 2] * a[..., 3] + b[..., 2] * b[..., 3] - inter)


def conditions(rec, convs, heads, truth, net, zero_gap=True):
    """whether one detailed call of the reference stays inside the conditions, and the margins (``zero_gap`` False: the
    leaky condition is the shipped case's cap on flipped masks instead, see make_shipped)"""
    zero = 1.0
    for n, l in enumerate(convs):
        if l["leaky"] and zero_gap:
            o = rec["fwd.conv%d.output" % n].astype(np.float64)
            pre = np.where(o > 0, o, o / .1)
            zero = min(zero, float(np.abs(pre).min()))
    gi = ga = gc = 1.0
    nw, nh = net["width"], net["height"]
    anc = np.asarray(heads[0]["head"]["anchors"], np.float64)
    anchors = np.stack([np.zeros(len(anc)), np.zeros(len(anc)), anc[:, 0] / nw, anc[:, 1] / nh], -1)
    hi = 0
    for n, l in enumerate(convs):
        if not l.get("is_head"):
            continue
        p = heads[hi]["head"]
        hi += 1
        x = rec["fwd.conv%d.output" % n].astype(np.float64)
        B, _, h, w = x.shape
        a = x.reshape(B, len(p["mask"]), 5 + p["classes"], h, w)
        jj, ii = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        sg = lambda v: 1. / (1. + np.exp(-v))
        aw, ah = anc[p["mask"], 0][None, :, None, None], anc[p["mask"], 1][None, :, None, None]
        pred = np.stack([(ii + sg(a[:, :, 0])) / w, (jj + sg(a[:, :, 1])) / h, np.exp(a[:, :, 2]) * aw / nw, np.exp(a[:, :, 3]) * ah / nh], -1)
        for b in range(B):
            rows = np.array([t for t in truth[b] if t[0] != 0], np.float64).reshape(-1, 5)
            if not len(rows):
                continue
            best = iou64(pred[b][..., None, :], rows[:, :4]).max(-1)
            gi = min(gi, float(np.abs(best - p["ignore_thresh"]).min()))
            for t in rows:
                s = np.sort(iou64(anchors, np.array([0, 0, t[2], t[3]])))
                ga = min(ga, float(s[-1] - s[-2]))
                fx, fy = t[0] * w, t[1] * h
                gc = min(gc, abs(fx - round(fx)), abs(fy - round(fy)))
    return (zero > EPS_ZERO or not zero_gap) and gi > EPS_IOU and ga > EPS_ANCHOR and gc > EPS_CELL, dict(zero=zero, iou=gi, anchor=ga, cell=gc)


TINY_WIDE_SEED = 900


def tiny_wide():
    """case a0's net (batch 3, one class) on a 24 x 16 input, from one seed: (cfg text, parameters, batch, truth)"""
    text = tiny_cfg(24, 16, 3, 1, 1, NET_A)
    return (text,) + seeded_inputs(TINY_WIDE_SEED, text)


def tiny_wide_step(device=None):
    """one train_step of tiny_wide's net: (quantities under case a0's names -- the cost, every convolution's output,
    batch mean and variance, the state after the update --, the heads' deltas)"""
    from betapose_amd.darknet_train import TrainableDarknet
    text, st, x, t = tiny_wide()
    net = TrainableDarknet(text, device=device)
    net.load_state(st)
    as_np = lambda a: np.array(a) if isinstance(a, np.ndarray) else a.cpu().numpy()
    q = {"a0.0.cost": np.float32(net.train_step(x, t))}
    for n, l in enumerate(net.convs):
        q["a0.0.fwd.conv%d.output" % n] = as_np(l["output"])
        if l["bn"]:
            q["a0.0.fwd.conv%d.mean" % n], q["a0.0.fwd.conv%d.variance" % n] = as_np(l["mean"]), as_np(l["variance"])
    q.update({"a0.0.post." + k: v for k, v in net.state().items()})
    return q, [as_np(d) for d in net.last_deltas]


# ---------------------------------------------------------------------------------------------------- the shipped topology
NET_A = "learning_rate=0.01\nburn_in=3\npolicy=steps\nsteps=2,10\nscales=.5,.1\nmax_batches=100\n"
SHIPPED = "darknet_train_shipped"
FLIP_CAP = 1e-4         # leaky outputs whose sign may differ between a float32 run and the free float64 run, of all


def shipped_cfg():
    """cfg.yolov3_single_cfg_text(1), random=0, on a 64 x 32 input with batch 2: 75 convolutions up to 1024 channels,
    heads on 2 x 1, 4 x 2 and 8 x 4 maps"""
    from betapose_amd import cfg as C
    body = C.yolov3_single_cfg_text(1)
    assert body.count("random=1") == 3
    return ("[net]\nbatch=2\nsubdivisions=1\nwidth=64\nheight=32\nchannels=3\nmomentum=0.9\ndecay=0.0005\n" + NET_A + "\n" +
            body.replace("random=1", "random=0"))


def parsed(text):
    """(net options, layers, convolutions, yolo layers) of a cfg text; the convolution before a head is marked"""
    from betapose_amd import cfg as C
    from betapose_amd.darknet_train import parse_layers
    net, layers = parse_layers(C.parse_cfg_text(text))
    for i, l in enumerate(layers):
        if l["type"] == "yolo":
            layers[i - 1]["is_head"] = True
    return net, layers, [l for l in layers if l["type"] == "convolutional"], [l for l in layers if l["type"] == "yolo"]


def seeded_state(rng, convs, classes):
    """initial parameters of modest scale: filters N(0, 1 / fan-in), heads with modest box terms and objectness -2"""
    f32 = np.float32
    st = {}
    for n, l in enumerate(convs):
        K, c, s = l["out"][0], l["cin"], l["size"]
        p = "conv%d." % n
        if l["bn"]:
            st[p + "weights"] = rng.normal(0, 1.0 / np.sqrt(c * s * s), (K, c, s, s)).astype(f32)
            st[p + "biases"] = rng.normal(0, .2, K).astype(f32)
            st[p + "scales"] = rng.uniform(.8, 1.2, K).astype(f32)
            st[p + "rolling_mean"] = rng.normal(0, .3, K).astype(f32)
            st[p + "rolling_variance"] = rng.uniform(.5, 1.5, K).astype(f32)
        else:       # a head: modest box terms, objectness biased low
            scale = np.tile(np.array([.5, .5, .15, .15, .6] + [.4] * classes, f32), 3)
            st[p + "weights"] = (rng.normal(0, 1, (K, c, 1, 1)).astype(f32) * scale[:, None, None, None]).astype(f32)
            st[p + "biases"] = np.tile(np.array([0, 0, 0, 0, -2.0] + [0.0] * classes, f32), 3)
    return st


def params_sha256(st):
    import hashlib
    h = hashlib.sha256()
    for k in sorted(st):
        h.update(k.encode() + np.ascontiguousarray(st[k], np.float32).tobytes())
    return h.hexdigest()


def seeded_inputs(seed, text):
    """(initial parameters, input batch, truth [B, 90, 5]) of the net of cfg ``text`` from one seed: seeded_state, a
    uniform image, per image two boxes then one, sized about the six smallest anchors and at most .9 of the image"""
    net, _, convs, heads = parsed(text)
    rng = np.random.default_rng([seed, net["width"], net["height"], net["batch"]])
    classes, anchors = heads[0]["head"]["classes"], np.asarray(heads[0]["head"]["anchors"], np.float64)
    st = seeded_state(rng, convs, classes)
    x = rng.uniform(0, 1, (net["batch"], net["channels"], net["height"], net["width"])).astype(np.float32)
    t = np.zeros((net["batch"], MAX_BOXES, 5), np.float32)
    for b in range(net["batch"]):
        for k in range(2 if b % 2 == 0 else 1):
            a = anchors[rng.integers(0, min(6, len(anchors)))] * rng.uniform(.8, 1.2, 2)
            t[b, k] = (rng.uniform(.15, .85), rng.uniform(.15, .85), min(a[0] / net["width"], .9), min(a[1] / net["height"], .9),
                       rng.integers(0, classes))
    return st, x, t


def leaky_masks(net):
    """per convolution of a TrainableDarknet after forward: where its leaky output is positive (None for a linear one)"""
    get = lambda a: np.asarray(a) if isinstance(a, np.ndarray) else a.cpu().numpy()
    return [get(l["output"]) > 0 if l["leaky"] else None for l in net.convs]


def shipped_inputs():
    """the shipped-topology case from the archive's seed; the archive's checksum of the parameter bytes is asserted, so a
    change of numpy's generator is reported as that and not as a numeric failure"""
    m, g = meta(SHIPPED), golden(SHIPPED)
    assert m["cfg"] == shipped_cfg(), "cfg.yolov3_single_cfg_text() is no longer the text the archive was made with"
    st, x, t = seeded_inputs(m["seed"], m["cfg"])
    assert params_sha256(st) == m["params_sha256"], "numpy's generator no longer gives the parameters the archive was made with"
    assert np.array_equal(t[:, :g["truth"].shape[1]], g["truth"]) and not t[:, g["truth"].shape[1]:].any()
    return st, x, t


def shipped_net(device=None):
    from betapose_amd.darknet_train import TrainableDarknet
    net = TrainableDarknet(meta(SHIPPED)["cfg"], device=device)
    net.load_state(shipped_inputs()[0])
    return net


def shipped_step(net):
    """group_a_step on the shipped topology: (quantities, the heads' own deltas, the leaky masks, a dict of the step's
    seconds and the update table's rows and blocks)"""
    import time
    g = golden(SHIPPED)
    _, x, t = shipped_inputs()
    t0 = time.perf_counter()
    q, deltas = step_in_parts(net, "shipped", x, t, [g["shipped.0.yolo%d.delta" % h] for h in range(len(net.heads))])
    return q, deltas, leaky_masks(net), dict(seconds=time.perf_counter() - t0, rows=net._ntab, blocks=net._blocks, net=net)


@functools.lru_cache(maxsize=None)
def shipped_host():
    """the host twin's step, once for the tests of both sides"""
    return shipped_step(shipped_net())


@functools.lru_cache(maxsize=None)
def shipped_host_second_cost():
    """the cost of a second call on the same batch, train_step forming its own deltas from the truth rows, on the net
    shipped_host() left behind (whose recorded quantities are copies)"""
    _, x, t = shipped_inputs()
    return np.float32(shipped_host()[3]["net"].train_step(x, t))


def f64_quantities(text, st, x, name, fed=None, truth=None, masks=None, blas=True):
    """one F64Net step under the quantity names of case ``name``: (quantities, (flips, leaky outputs) of ``masks``
    against the free float64 forward).  ``masks`` teacher-force the backward pass."""
    from darknet_train_f64 import F64Net, mask_flips
    net, layers, _, _ = parsed(text)
    ex = F64Net(net, layers, st, blas=blas)
    cost, rec, pre = ex.step(x, fed, truth, masks)
    q = {"%s.0.fwd.%s" % (name, k): v for k, v in rec.items()}
    q.update({"%s.0.pre.%s" % (name, k): v for k, v in pre.items()})
    q.update({"%s.0.post.%s" % (name, k): v for k, v in ex.st.items()})
    if cost is not None:
        q["%s.0.cost" % name] = cost
    return q, (mask_flips(masks, ex.masks()) if masks is not None else (0, 0))


@functools.lru_cache(maxsize=None)
def shipped_exact():
    """the float64 step fed the reference's deltas and teacher-forced on the host twin's masks (the device's are the
    same bits), once: (quantities, (flips, leaky outputs))"""
    g = golden(SHIPPED)
    st, x, _ = shipped_inputs()
    fed = [g["shipped.0.yolo%d.delta" % h] for h in range(3)]
    return f64_quantities(meta(SHIPPED)["cfg"], st, x, "shipped", fed, masks=shipped_host()[2])


def check_shipped(q, label):
    """every quantity of a shipped-topology step within its bar of the float64 step; prints the worst distance / bar"""
    exact, (flips, leaky) = shipped_exact()
    print("%s: %d of %d leaky outputs differ in sign from the free float64 run (cap %d, the reference's own %d)"
          % (label, flips, leaky, int(FLIP_CAP * leaky), meta(SHIPPED)["mask_flips"]))
    assert flips <= FLIP_CAP * leaky
    assert set(exact) <= set(q) and len(exact) > 600
    worst = max((check(k, q[k], against=v, archive=SHIPPED, quiet=True), k) for k, v in exact.items())
    print("%s: %d quantities, worst distance / bar %.3f at %s" % (label, len(exact), worst[0], worst[1]))


# ---------------------------------------------------------------------------------------------------- kernels alone
# name, N, Cin, H, W, Cout, size, stride: neither channel count a multiple of a tile, 1 x 1 and 3 x 3, stride 2 on odd
# sizes, a 2 x 2 map, K = 720 (several k steps and a partial last one), N 1 and 3, a filter gradient over more than one
# reduction slice (3 * 26 * 26 = 2028 < 2048 < 3 * 27 * 27) and one that does not fill the first
CONV_SHAPES = [("c3_k18_3x3", 3, 3, 9, 11, 18, 3, 1), ("c3_k18_1x1", 1, 3, 6, 5, 18, 1, 1), ("s2_13", 1, 5, 13, 13, 7, 3, 2),
               ("s2_5x7", 3, 4, 5, 7, 6, 3, 2), ("map2x2", 3, 6, 2, 2, 5, 3, 1), ("c80", 1, 80, 4, 5, 18, 3, 1),
               ("s2_1x1", 1, 9, 7, 6, 4, 1, 2), ("slices", 3, 3, 27, 27, 18, 3, 1), ("wide", 1, 3, 8, 9, 70, 1, 1)]
# the layer shapes of cfg.yolov3_single_cfg_text() on the smallest maps that keep each property: 16 block rows over one
# partial block column with chains of 4608 (forward) and 9216 terms (input gradient), the bottleneck 1 x 1 on a 2 x 1 map,
# Cin = 768 after `route -1, 61`, a down-sampling layer onto a 2 x 1 map, the heads' M = 18 and M = 255 against 64-row
# tiles; then the filter gradient's slices of 2048: six with a last one of 128, stride 2 on odd unequal sides, one slice
# exactly full, two exactly full, and a second slice of one value
CONV_SHAPES += [("c512_k1024", 2, 512, 2, 2, 1024, 3, 1), ("c1024_k512_1x1", 2, 1024, 2, 1, 512, 1, 1),
                ("c768_k256_1x1", 1, 768, 4, 2, 256, 1, 1), ("c256_k512_s2", 2, 256, 4, 2, 512, 3, 2), ("head18", 2, 1024, 2, 1, 18, 1, 1),
                ("head255", 1, 256, 4, 4, 255, 1, 1), ("stem_6slices", 2, 3, 72, 72, 32, 3, 1), ("stem_s2_odd", 3, 32, 33, 31, 64, 3, 2),
                ("k2048", 2, 3, 32, 32, 18, 3, 1), ("k4096", 4, 3, 32, 32, 18, 3, 1), ("k2049", 3, 4, 1, 683, 5, 1, 1)]


def conv_case(shape, seed=7):
    """(x, w, delta of the output, a non-zero delta of the input, non-zero filter updates) of one shape"""
    _, N, C, H, W, K, size, stride = shape
    rng = np.random.default_rng([seed, N, C, H, W, K, size, stride])
    pad = size // 2
    OH, OW = (H + 2 * pad - size) // stride + 1, (W + 2 * pad - size) // stride + 1
    f = lambda *s: rng.normal(0, 1, s).astype(np.float32)
    return f(N, C, H, W), f(K, C, size, size), f(N, K, OH, OW), f(N, C, H, W), f(K, C, size, size)


def subnormal_conv_case():
    """c3_k18_3x3 with x, w and the output's delta scaled by 2^-70 and the values added into by 2^-140: every product
    and every partial sum of each role is subnormal or zero (the delta is scaled too, so that this holds in the two
    gradient roles, whose operands it is)"""
    shape = CONV_SHAPES[0]
    assert shape[0] == "c3_k18_3x3"
    x, w, dy, dx0, wu0 = conv_case(shape)
    a, b = np.float32(2.0 ** -70), np.float32(2.0 ** -140)
    return shape, x * a, w * a, dy * a, dx0 * b, wu0 * b


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
        return np.einsum("nctyx,kct->nkyx", cols, w.reshape(K, C, s * s), optimize=True)
    if role == 1:
        return wu0 + np.einsum("nkyx,nctyx->kct", dy, cols, optimize=True).reshape(w.shape)
    dc = np.einsum("nkyx,kct->nctyx", dy, w.reshape(K, C, s * s), optimize=True)
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


# N, C, S; the second row: a count of 2 and of 4 at 1024 channels, the two sides of the 256-lane stride, an odd long row
BN_SHAPES = [(1, 10, 4), (3, 10, 169), (3, 70, 4), (1, 70, 169),
             (2, 1024, 1), (2, 1024, 2), (1, 2, 256), (1, 2, 257), (3, 32, 1023)]


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
