"""fp64 numpy restatement of the two context-window passes (include/moviigen_hip.h) for tests/test_context_windows.py.
The weights are the fp32 ones the kernels read, widened: what is checked is the kernels' arithmetic, not the rounding of the weights."""
import numpy as np


def gather_ref(x, f0, Fw):
    """x [C, F, hw] -> the window [C, Fw, hw] at frames [f0, f0 + Fw): a slice, the same bits"""
    return np.ascontiguousarray(x[:, f0:f0 + Fw])


def blend_ref(preds, starts, weights, F):
    """preds: one [C, Fw, hw] fp32 array per window, starts: their first frames, weights: [K, Fw] fp32 ->
    (value, mag, count): value [C, F, hw] fp64 = sum_k w_k v_k over the windows that cover a frame, mag = sum_k w_k |v_k|, count [F] = the
    number of windows that cover a frame (NaN / 0 where none does)"""
    C, Fw, hw = preds[0].shape
    value, mag, count = np.zeros((C, F, hw)), np.zeros((C, F, hw)), np.zeros(F, dtype=np.int64)
    for v, f0, w in zip(preds, starts, np.asarray(weights, dtype=np.float64)):
        value[:, f0:f0 + Fw] += w[None, :, None] * v.astype(np.float64)
        mag[:, f0:f0 + Fw] += w[None, :, None] * np.abs(v.astype(np.float64))
        count[f0:f0 + Fw] += 1
    value[:, count == 0] = np.nan
    return value, mag, count


def blend_once_ref(acc, pred, f0, w, first):
    """one call: acc [C, F, hw] fp32, pred [C, Fw, hw] fp32, w [Fw] fp32, first [Fw] -> (value fp64 [C, F, hw], mag): inside the window
    w v where first (acc is not read), w v + a elsewhere; outside the window acc itself"""
    value, mag = acc.astype(np.float64), np.abs(acc.astype(np.float64))
    Fw = pred.shape[1]
    wv = np.asarray(w, dtype=np.float64)[None, :, None] * pred.astype(np.float64)
    sel = np.asarray(first).astype(bool)[None, :, None]
    value[:, f0:f0 + Fw] = np.where(sel, wv, wv + value[:, f0:f0 + Fw])
    mag[:, f0:f0 + Fw] = np.where(sel, np.abs(wv), np.abs(wv) + mag[:, f0:f0 + Fw])
    return value, mag
