"""Direct-sum models of the FIR filter (include/sot_hip.h: sot_fir_same_forward / _backward) for the FIR tests: exact in int64 for
integer data, float64 for float data.  With x zero outside [0, T):
    y[b,t]  = sum_k h[b,k] x[b, t + start - k]
    gx[b,u] = sum_k h[b,k] g[b, u - start + k]
    gh[b,k] = sum_t g[b,t] x[b, t + start - k]
"""
import numpy as np


def default_start(taps: int) -> int:
    return (taps - 1) // 2 - 1


def _rows(h, batch):
    h = np.asarray(h)
    return np.broadcast_to(h, (batch, h.shape[-1])) if h.ndim == 1 else h


def forward(x, h, start):
    """[B, T] from x [B, T] and h [B, L] or [L]; the dtype of the inputs decides the arithmetic (int64 or float64)."""
    x = np.asarray(x)
    B, T = x.shape
    h = _rows(h, B)
    L = h.shape[1]
    out = np.zeros((B, T), dtype=np.result_type(x.dtype, h.dtype))
    for b in range(B):
        full = np.convolve(x[b], h[b])              # full[n] = sum_k h[k] x[n - k], n < T + L - 1
        out[b] = full[start:start + T]
    return out


def grad_audio(g, h, start):
    g = np.asarray(g)
    B, T = g.shape
    h = _rows(h, B)
    L = h.shape[1]
    return forward(g, h[:, ::-1], L - 1 - start)


def grad_taps(g, x, taps, start):
    """[B, L]: per clip (a shared filter's gradient is the sum over the clips)."""
    g, x = np.asarray(g), np.asarray(x)
    B, T = x.shape
    out = np.zeros((B, taps), dtype=np.result_type(g.dtype, x.dtype))
    for b in range(B):
        corr = np.correlate(g[b], x[b], mode="full")    # corr[j] = sum_t g[t + j - (T - 1)] x[t]  ->  lag d = j - (T - 1): sum_t g[t + d] x[t]
        for k in range(taps):
            d = k - start                                # gh[k] = sum_t g[t] x[t + start - k] = sum_u g[u + k - start] x[u]
            j = d + (T - 1)
            out[b, k] = corr[j] if 0 <= j < 2 * T - 1 else 0
    return out
