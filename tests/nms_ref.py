"""A plain f32 numpy restatement of the reference's live-NMS branch of ``write_results`` (yolo/util.py:118-196 with
``nms = True`` and without the final arg-max of :210-211) and of ``bbox_iou`` (yolo/bbox.py:51-77), op for op.  The
reference's own function cannot make fixtures for it (its switch is hard-coded off, its IoU calls ``.cuda()``), so
tests/test_candidates_host.py pins candidate 0 of this restatement to ``oracle.yolo_ref.write_results`` instead."""
import numpy as np

F32 = np.float32


def bbox_iou(box1, box2):
    """box1 [1,4+], box2 [m,4+] corner boxes, f32 -> iou [m] (the + 1 on widths and heights included)."""
    b1 = np.asarray(box1, F32)
    b2 = np.asarray(box2, F32)
    one, zero = F32(1), F32(0)
    with np.errstate(all="ignore"):
        ix1 = np.maximum(b1[:, 0], b2[:, 0])
        iy1 = np.maximum(b1[:, 1], b2[:, 1])
        ix2 = np.minimum(b1[:, 2], b2[:, 2])
        iy2 = np.minimum(b1[:, 3], b2[:, 3])
        inter = np.maximum(ix2 - ix1 + one, zero) * np.maximum(iy2 - iy1 + one, zero)
        a1 = (b1[:, 2] - b1[:, 0] + one) * (b1[:, 3] - b1[:, 1] + one)
        a2 = (b2[:, 2] - b2[:, 0] + one) * (b2[:, 3] - b2[:, 1] + one)
        return (inter / (a1 + a2 - inter)).astype(F32)


def select_nms(pred, confidence, num_classes, nms_conf, max_candidates, class_id=0, ious_out=None):
    """pred [B,rows,attrs] f32 -> (records [B,C,8] f32, counts [B] int32): per survivor (row index as int bits, x1, y1,
    x2, y2, objectness, class score, class id), unused slots index -1 and zeros.  Rows with objectness > confidence whose
    first-max class is ``class_id``, sorted by descending objectness (stable: the lower row first on ties); every kept
    row removes the later rows whose IoU with it is not < nms_conf.  ``ious_out``: a list that receives every IoU
    computed (the tests' margin precondition)."""
    pred = np.asarray(pred, F32)
    B, rows, attrs = pred.shape
    C = int(max_candidates)
    out = np.zeros((B, C, 8), F32)
    out[:, :, 0] = np.array([-1], np.int32).view(F32)[0]
    counts = np.zeros(B, np.int32)
    ncls = min(int(num_classes), attrs - 5)
    for b in range(B):
        p = pred[b]
        rows_live = np.nonzero(p[:, 4] > F32(confidence))[0]
        if rows_live.size == 0:
            continue
        cls = np.argmax(p[rows_live, 5:5 + ncls], axis=1)          # first maximum
        rows_live = rows_live[cls == class_id]
        if rows_live.size == 0:
            continue
        two = F32(2)
        box = np.stack([p[rows_live, 0] - p[rows_live, 2] / two, p[rows_live, 1] - p[rows_live, 3] / two,
                        p[rows_live, 0] + p[rows_live, 2] / two, p[rows_live, 1] + p[rows_live, 3] / two], 1).astype(F32)
        order = np.argsort(-p[rows_live, 4], kind="stable")
        rows_live, box = rows_live[order], box[order]
        kept = 0
        while rows_live.size and kept < C:
            r = rows_live[0]
            out[b, kept, 0] = np.array([r], np.int32).view(F32)[0]
            out[b, kept, 1:5] = box[0]
            out[b, kept, 5] = p[r, 4]
            out[b, kept, 6] = p[r, 5 + class_id]
            out[b, kept, 7] = F32(class_id)
            kept += 1
            if rows_live.size == 1:
                break
            ious = bbox_iou(box[:1], box[1:])
            if ious_out is not None:
                ious_out.append(ious)
            keep = ious < F32(nms_conf)                              # a NaN IoU removes
            rows_live, box = rows_live[1:][keep], box[1:][keep]
        counts[b] = kept
    return out, counts
