#!/usr/bin/env python3
"""The convolution plan of both networks and of the cfgs of tests/cfg_topologies.py, as Net::profile reports it: per
configuration the (tile, K slices) of every op and the number of fused launches.  tests/golden/conv_plan.json pins it
(tests/test_gpu_conv_plan.py); a pull request that retunes on purpose regenerates the fixture:

    python tools/dump_conv_plan.py            # compare with the fixture, print what differs
    python tools/dump_conv_plan.py --write    # rewrite the fixture

Needs a GPU: the rows come from an eager profiling pass (profile(batch, 1)) of an engine in that configuration."""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
FIXTURE = os.path.join(ROOT, "tests", "golden", "conv_plan.json")
MODES = ("f32", "bf16x3", "f16", "f16r")
NETWORKS = ("yolo", "kpd")
POLICY = (256, 8, 16)       # the one explicit split-K policy of the record: target blocks, min chunks per slice, max slices


def topologies():
    import cfg_topologies as T
    return sorted(T.CASES)


def make_net(network, mode, directory=None):
    """A fresh engine in `mode`: the two networks with room for 28 frames, a cfg of tests/cfg_topologies.py for 3."""
    import helpers
    if network == "yolo":
        from betapose_amd.darknet import Darknet
        net = Darknet("yolo/cfg/yolov3-single.cfg", reso=416, max_batch=28).load_stream(helpers.yolo_stream()).cuda().eval()
    elif network == "kpd":
        from betapose_amd.kpd import FastPoseHIP
        net = FastPoseHIP(helpers.kpd_state_dict(), n_classes=50, max_batch=28).cuda().eval()
    else:
        import cfg_topologies as T
        return T.make_net(network, directory or tempfile.mkdtemp(), mode)
    net.set_precision(mode)
    return net


def rows(net, batch):
    """What the engine would launch now: [tile, slices, tile, slices, ...] over the ops, and the fused launches."""
    info = net.profile(batch, 1)[1]
    return {"rows": [int(v) for v in info[:, [1, 3]].reshape(-1)], "fused": net.fused_launches(batch)}


def record(net, network, mode):
    """Every configuration of the record for one engine, which is in `mode` under the default policy and is left so."""
    big = network in NETWORKS
    out = {}
    for b in ((1, 2, 4, 28) if big else (1, 2)):
        out["b%d" % b] = rows(net, b)
    if not big:
        return out
    if mode in ("bf16x3", "f16"):            # the lone-frame rows, and the unfused plan
        net.set_prefetch(True)
        out["b1_prefetch"] = rows(net, 1)
        net.set_prefetch(False)
        net.set_fusion(False)
        for b in (1, 28):
            out["b%d_unfused" % b] = rows(net, b)
        net.set_fusion(True)
    if mode in ("f32", "f16"):
        net.set_policy(*POLICY)
        for b in (1, 28):
            out["b%d_policy" % b] = rows(net, b)
        net.set_policy()
    if mode in ("f16", "bf16x3"):
        net.set_policy(force_tile=13 if mode == "f16" else 0)
        out["b1_force"] = rows(net, 1)
        net.set_policy()
    return out


def load():
    with open(FIXTURE) as f:
        return json.load(f)


def main():
    networks = NETWORKS + tuple(topologies())
    plan = {n: {m: record(make_net(n, m), n, m) for m in MODES} for n in networks}
    if "--write" in sys.argv:
        with open(FIXTURE, "w") as f:       # one configuration per line, integers only
            f.write("{\n" + ",\n".join(
                '"%s": {\n' % n + ",\n".join(
                    ' "%s": {\n' % m + ",\n".join('  "%s": %s' % (k, json.dumps(v, separators=(",", ":"))) for k, v in plan[n][m].items()) + "}"
                    for m in MODES) + "}"
                for n in networks) + "}\n")
        print("wrote %s: %d bytes" % (FIXTURE, os.path.getsize(FIXTURE)))
        return 0
    want, bad = load(), 0
    for n in networks:
        for m in MODES:
            for k, v in plan[n][m].items():
                if want.get(n, {}).get(m, {}).get(k) != v:
                    bad += 1
                    print("differs from the fixture: %s %s %s" % (n, m, k))
    print("%d configurations differ" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
