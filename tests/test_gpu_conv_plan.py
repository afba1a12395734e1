"""The convolution plan as a whole, pinned: which kernel runs every op of both networks and of the cfgs of cfg_topologies.py, with how
many K slices, and how many blocks run fused -- in every precision, at several batch sizes, under an explicit policy, a forced tile and
the lone-frame mode (tests/golden/conv_plan.json, written by tools/dump_conv_plan.py --write from the engine as it was before the
planner became a module of its own).  A pull request that moves a layer to another kernel shows up here; one that does so on
purpose regenerates the fixture.  And the plan the engine caches per batch size is never a stale one."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dump_conv_plan as D  # noqa: E402

_FIXTURE = {}


def fixture():
    if not _FIXTURE:
        _FIXTURE.update(D.load())
    return _FIXTURE


@pytest.mark.parametrize("mode", D.MODES)
@pytest.mark.parametrize("network", D.NETWORKS + tuple(D.topologies()))
def test_plan_equals_the_record(cuda, tmp_path, network, mode):
    want = fixture()[network][mode]
    got = D.record(D.make_net(network, mode, tmp_path), network, mode)
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key]["fused"] == want[key]["fused"], (network, mode, key)
        assert got[key]["rows"] == want[key]["rows"], (network, mode, key, _first_difference(got[key]["rows"], want[key]["rows"]))


def _first_difference(got, want):
    for i in range(0, min(len(got), len(want)), 2):
        if got[i:i + 2] != want[i:i + 2]:
            return "op %d: (tile, slices) %s, recorded %s" % (i // 2, got[i:i + 2], want[i:i + 2])
    return "%d ops, recorded %d" % (len(got) // 2, len(want) // 2)


@pytest.mark.parametrize("network", D.NETWORKS)
def test_no_stale_plan_on_one_engine(cuda, network):
    """One engine through precisions, batch sizes, policies, the lone-frame mode and the fusion switch: after every step the rows are
    the record's rows for that configuration (fresh engines wrote it), and a batch-1 forward between batch-28 forwards gives the bits a
    fresh engine gives."""
    fix = fixture()[network]
    net = D.make_net(network, "f16")
    shape = (28, 3, 416, 416) if network == "yolo" else (28, 3, 320, 256)
    x = torch.rand(shape, generator=torch.Generator().manual_seed(77)).to(cuda)

    def check(step, mode, **keys):       # batch -> the record's key
        for batch, key in keys.items():
            assert D.rows(net, int(batch[1:])) == fix[mode][key], (step, mode, key)

    check(1, "f16", b28="b28")
    net(x)
    net.set_precision("bf16x3")
    check(2, "bf16x3", b28="b28")
    net.set_precision("f16")
    check(3, "f16", b1="b1")
    one = net(x[:1]).clone()
    check(4, "f16", b28="b28")
    net(x)
    net.set_policy(*D.POLICY)
    check(5, "f16", b1="b1_policy", b28="b28_policy")
    net.set_policy()
    check(6, "f16", b1="b1", b28="b28")
    net.set_prefetch(True)
    check(7, "f16", b1="b1_prefetch")
    net.set_prefetch(False)
    check(8, "f16", b1="b1")
    net.set_fusion(False)
    check(9, "f16", b1="b1_unfused", b28="b28_unfused")
    net.set_fusion(True)
    check(10, "f16", b1="b1", b28="b28")
    assert torch.equal(net(x[:1]), one)
    assert torch.equal(D.make_net(network, "f16")(x[:1]), one)
