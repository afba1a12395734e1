"""Planted frames shared by tests/test_instances_host.py and tests/test_gpu_instances.py: the candidate cases of
tests/test_gpu_candidates.py (imported, not copied) plus frames that exercise the per-instance poses -- several rigid
instances in one frame, a frame without candidates, one whose first pick is filtered and one whose every merged pose is.
Host-only: nothing here needs a GPU."""
import numpy as np

import test_gpu_candidates as tc  # noqa: E402  (builders only: _base_record, _shifted, _cases, _host_nms)
from betapose_amd import ops
from betapose_amd.synth import CAM_K, synth_kp3d

KP3D = synth_kp3d(50)
F32 = np.float32
RT_TOL = 1e-9


def pose_record(rng, rotvec, t, scores, index=5):
    """A record whose 50 arg-max pixels are the projection of KP3D under (rotvec, t), seen through a 200 x 250 crop
    window around them (tests/test_gpu_candidates.py _base_record with the pose as an argument)."""
    from scipy.spatial.transform import Rotation as Rot
    Y = KP3D @ Rot.from_rotvec(rotvec).as_matrix().T + np.asarray(t, np.float64)
    uv = Y @ CAM_K.T
    uv = uv[:, :2] / uv[:, 2:]
    rec = np.zeros(316, F32)
    rec[0] = np.array([index], np.int32).view(F32)[0]
    ul = np.round(uv.mean(axis=0) - np.array([110.0, 130.0])).astype(F32)
    br = ul + np.array([200.0, 250.0], F32)
    rec[1:5] = [10, 20, 30, 40]
    rec[5] = 0.875
    rec[8:10], rec[10:12] = ul, br
    rec[12:16] = [ul[0] + 5, ul[1] + 7, br[0] - 4, br[1] - 6]
    hx = np.clip(np.round((uv[:, 0] - ul[0]) * 80 / 250 - 0.2), 1, 62).astype(np.int32)
    hy = np.clip(np.round((uv[:, 1] - ul[1]) * 80 / 250 - 0.2), 1, 78).astype(np.int32)
    kp = rec[16:].reshape(50, 6)
    kp[:, 0] = (hy * 64 + hx).astype(np.int32).view(F32)
    kp[:, 1] = rng.uniform(scores[0], scores[1], 50).astype(F32)
    kp[:, 2:] = rng.uniform(0, 0.3, (50, 4)).astype(F32)
    return rec


def rigid_case(n, seed):
    """n instances of the object side by side, each the projection of its own rigid pose: n merged poses, each a
    well-posed PnP.  Candidate 0 has the highest mean score; the others come in falling order of theirs."""
    rng = np.random.default_rng(seed)
    recs = []
    for c in range(n):
        rotvec = np.array([0.3, -0.5, 0.2]) + 0.15 * rng.normal(size=3)
        t = np.array([-0.45 + 0.13 * c, -0.03 + 0.02 * (c % 3), 0.8 + 0.03 * c])
        hi = 0.95 - 0.05 * c
        recs.append(pose_record(rng, rotvec, t, (hi - 0.1, hi), index=5 + c))
    return np.array(recs)


# Seeds chosen on the HOST solver alone: the first ones at which every instance's one-ulp movement (tests/
# test_gpu_pose_tail.py _one_ulp_sensitivity, left_number 50 and 10) stays below RT_TOL / 10, so that the host bar of the GPU
# test is never met through the ill-conditioning rule.  (Key points are heat-map pixels, 3 px apart: the 20-step minimiser
# stops short of convergence on most eight-instance frames, and its last bits then move by 1e-9 and more.)
RIGID_SEEDS = ((2, 300), (3, 300), (8, 306))
# Existing planted frames whose instances j > 0 move by RT_TOL / 10 or more under a one-ulp change at this left_number
# (measured: 'far n=8' 5.6e-9, 'below n=8' 1.5e-9): held to the device solver bit for bit, not to the host bar.
HOST_BAR_EXCLUDED = {("far n=8", 10), ("below n=8", 10)}


def all_filtered_case():
    """Two far-apart candidates, no key-point score of either reaches 0.3: every merged pose is filtered (status 2)."""
    rng = np.random.default_rng(21)
    a = tc._base_record(rng, scores=(0.1, 0.29))
    return np.array([a, tc._shifted(a, rng, 150.0, 0.0, 0.0, (0.05, 0.2))])


def cases():
    """[(name, records [n, 316])]: the existing planted cases (m = 1, 2, 3, 8; 'two clusters'; 'first pick filtered'),
    the rigid family at n = 2, 3, 8, the all-filtered frame and a frame without candidates (n = 0)."""
    out = list(tc._cases())
    for n, seed in RIGID_SEEDS:
        out.append(("rigid n=%d" % n, rigid_case(n, seed)))
    out.append(("all filtered", all_filtered_case()))
    out.append(("no candidate", np.zeros((0, 316), F32)))
    return out


def cases_for(C):
    """The cases that fit a launch at C candidates per frame; at C = 1 also the first candidate alone of a few frames."""
    cs = cases()
    keep = [(nm, r) for nm, r in cs if len(r) <= C]
    if C == 1:
        keep += [(nm + " [:1]", r[:1]) for nm, r in cs if nm in ("rigid n=2", "two clusters", "first pick filtered", "all filtered")]
    return keep


def pack(keep, C):
    """Cases of at most C candidates as launch inputs: (names, records [F, C, 316], counts [F])."""
    assert all(len(r) <= C for _, r in keep)
    recs = np.zeros((len(keep), C, 316), F32)
    recs[:, :, 0] = np.array([-1], np.int32).view(F32)[0]
    counts = np.zeros(len(keep), np.int32)
    for i, (_, r) in enumerate(keep):
        recs[i, :len(r)] = r
        counts[i] = len(r)
    return [nm for nm, _ in keep], recs, counts


def pruned_points(keypoints, kp_score, left):
    """The reference's pruning loop (dataloader.py:718-722) on one merged pose -> (kp_3d [p, 3], kp_2d [p, 2]) f64."""
    sc = np.array(kp_score, F32).reshape(-1)
    k2 = np.array(keypoints, F32)
    k3 = np.array(KP3D)
    while len(k2) > left:
        d = int(np.argmin(sc))
        sc, k2, k3 = np.delete(sc, d), np.delete(k2, d, axis=0), np.delete(k3, d, axis=0)
    return k3, k2.astype(np.float64)


def host_instance_pose(human, left):
    """ops.solve_pnp on a merged pose's pruned points."""
    k3, k2 = pruned_points(human["keypoints"], human["kp_score"], left)
    return ops.solve_pnp(k3, k2, CAM_K)
