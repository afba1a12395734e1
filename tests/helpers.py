"""Shared test inputs: the same seeded synthetic weights / frames the golden
fixtures were generated from (tools/make_golden.py)."""
import functools
import os
import re

import numpy as np

from betapose_amd import cfg as C, synth, weights as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
YOLO_SEED, KPD_SEED, FRAME_SEED = 1, 2, 1234


@functools.lru_cache(None)
def yolo_blocks():
    return C.parse_cfg_text(C.yolov3_single_cfg_text())


@functools.lru_cache(None)
def yolo_stream():
    return synth.synth_yolo_stream(YOLO_SEED, yolo_blocks())


@functools.lru_cache(None)
def kpd_state_dict():
    return synth.synth_fastpose_state_dict(KPD_SEED)


@functools.lru_cache(None)
def frames(n=4):
    return synth.synth_frames(n, FRAME_SEED)


@functools.lru_cache(None)
def header_code():
    """include/betapose_hip.h with its comments stripped: what the compiler sees of the C ABI."""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "betapose_hip.h")).read(), flags=re.S)


def header_names():
    """Every ``bp_*`` function the header declares."""
    return set(re.findall(r"\b(bp_[a-z0-9_]+)\s*\(", header_code()))


def golden(name):
    return np.load(os.path.join(GOLD, name), allow_pickle=False)


def yolo_input_from_frame(frame_bgr, reso=416):
    """a1 on the host exactly as the reference does it: PIL bicubic stretch + ToTensor
    (dataloader.py:94-99,162)."""
    import torch
    from PIL import Image
    img = Image.fromarray(np.ascontiguousarray(frame_bgr[:, :, ::-1])).resize((reso, reso), 3)
    a = np.asarray(img, dtype=np.uint8).transpose(2, 0, 1).copy()
    return torch.from_numpy(a).float().div(255).unsqueeze(0)


class CountingSource:
    """An in-memory frame source with ``FrameLoader``'s surface for the runners: yields ``(i, frame, host address)`` and
    records every ``release(i)``, so a test can tell that each slot it handed out came back exactly once."""

    def __init__(self, frame_list):
        self.frames = [np.ascontiguousarray(f) for f in frame_list]
        self.yielded, self.released = [], []

    def __iter__(self):
        for i, f in enumerate(self.frames):
            self.yielded.append(i)
            yield i, f, f.ctypes.data

    def release(self, i):
        self.released.append(i)

    def assert_each_released_once(self):
        assert sorted(self.released) == self.yielded, (self.yielded, self.released)
