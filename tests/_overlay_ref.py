"""The numpy float32 evaluation of vk_stroke_overlay_u8's definition (include/vista_hip.h), written before the kernel: the kernel's bytes must
equal this file's, without a tolerance. Every operation below is one numpy float32 operation -- rounded once, nothing fused.

A stroke is (colour (3 floats in [0, 255]), alpha, r, segments); a segment is (ax, ay, bx, by), a disc a segment with a == b. A stroke set is a
list of strokes, drawn in list order. Per pixel centre p = (x + 0.5, y + 0.5):
    d    = b - a                         inv_len2 = 0 for a disc, else 1 / (d.x * d.x + d.y * d.y)          (formed once per segment)
    t    = clamp(((p.x - a.x) * d.x + (p.y - a.y) * d.y) * inv_len2, 0, 1)
    q    = a + t * d                     e = p - q                  dist = sqrt(e.x * e.x + e.y * e.y)
    cov  = clamp((r + 0.5) - dist, 0, 1)                            a stroke's coverage: the maximum over its segments
    f   <- f + (alpha * cov) * (K - f)   per channel, strokes in list order, starting from float(byte); the final cast truncates.
"""
import numpy as np

F = np.float32


def inv_len2(ax, ay, bx, by):
    """What the host hands the kernel with every segment: 1 / |b - a|^2 in float32, 0 for a disc."""
    dx, dy = F(bx) - F(ax), F(by) - F(ay)
    l2 = dx * dx + dy * dy
    return F(0) if l2 == 0 else F(1) / l2


def coverage(H, W, r, segments):
    """(H, W) float32: the stroke's coverage of every pixel; zeros for a stroke without segments."""
    py, px = np.meshgrid(np.arange(H, dtype=F) + F(0.5), np.arange(W, dtype=F) + F(0.5), indexing="ij")
    cov = np.zeros((H, W), dtype=F)
    rh = F(r) + F(0.5)
    for ax, ay, bx, by in segments:
        ax, ay = F(ax), F(ay)
        dx, dy = F(bx) - ax, F(by) - ay
        il2 = inv_len2(ax, ay, bx, by)
        dot = (px - ax) * dx + (py - ay) * dy
        t = np.minimum(np.maximum(dot * il2, F(0)), F(1))
        qx, qy = ax + t * dx, ay + t * dy
        ex, ey = px - qx, py - qy
        dist = np.sqrt(ex * ex + ey * ey)
        c = np.minimum(np.maximum(rh - dist, F(0)), F(1))
        assert c.dtype == F
        cov = np.maximum(cov, c)
    return cov


def draw(frame, strokes):
    """One (H, W, 3) uint8 frame under a list of strokes -> a new (H, W, 3) uint8 frame."""
    H, W, _ = frame.shape
    f = frame.astype(F)
    for colour, alpha, r, segments in strokes:
        a = F(alpha) * coverage(H, W, r, segments)
        for c in range(3):
            diff = F(colour[c]) - f[..., c]
            f[..., c] = f[..., c] + a * diff
    assert f.dtype == F
    return f.astype(np.int32).astype(np.uint8)


def overlay(frames, sets, set_of_frame):
    """(n, H, W, 3) uint8 frames; frame i is drawn with sets[set_of_frame[i]], or copied where set_of_frame[i] is outside [0, len(sets))."""
    out = np.array(frames, dtype=np.uint8, copy=True)
    for i, s in enumerate(set_of_frame):
        if 0 <= int(s) < len(sets):
            out[i] = draw(frames[i], sets[int(s)])
    return out
