"""Shared by test_tracking_static_cpu.py and test_tracking_static_gpu.py: padded step inputs whose padding is a trap."""
import numpy as np


def padded(frames_of_segments, cap, trap_label):
    """one step's padded inputs (boxes [S, cap, 9], labels, scores [S, cap], counts [S]) from one frame dictionary per segment.  The rows
    behind counts[s] are a trap - NaN boxes, a label that is a tracking class, score 1.0: any read past the count changes ids or the
    track list."""
    s = len(frames_of_segments)
    boxes = np.full((s, cap, 9), np.nan, np.float32)
    labels, scores = np.full((s, cap), trap_label, np.int64), np.ones((s, cap), np.float32)
    counts = np.array([len(f["boxes"]) for f in frames_of_segments], np.int32)
    for i, f in enumerate(frames_of_segments):
        boxes[i, :counts[i]], labels[i, :counts[i]], scores[i, :counts[i]] = f["boxes"], f["labels"], f["scores"]
    return boxes, labels, scores, counts
