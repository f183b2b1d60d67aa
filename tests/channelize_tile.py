"""The tile of the wideband front end's kernels (k_channelize.hip: channelize_outputs_per_lane and rechannelize_shape), restated for
the tests that cut their captures around it.  span_bytes is the size of one span element in LDS: 8 for an analytic capture (float2),
4 for a real one (float)."""
import math


def tile_shape(P, Q, span_bytes):
    """-> (outputs of one workgroup's tile, outputs or slots per lane).  Q = 1: 64 R outputs, R = 4 but 2 for an analytic D > 16.
    Else Q M, with M outputs per residue - as many as leave four waves' phasors and the span [P][odd rows] inside 64 KiB of LDS, and at
    most 64 NP / Q for NP slots per lane, NP the largest of 4 .. 1 at which 85 % of the slots hold an output"""
    assert span_bytes in (4, 8)
    if Q == 1:
        per_lane = 2 if span_bytes == 8 and P > 16 else 4
        return 64 * per_lane, per_lane
    T = 24 * P // Q + 1
    hist = -(-(T - 1) // P)
    rows = (65536 - 32 * T) // span_bytes // P
    rows -= 1 - rows % 2
    for passes in (4, 3, 2, 1):
        m = min(64 * passes // Q, rows - hist)
        if 100 * Q * m >= 85 * 64 * passes:
            break
    return Q * m, passes


def admitted_ratios():
    """every p / q in lowest terms the ratio form admits: 2 <= q <= 16, 2 <= p / q <= 32"""
    return [(p, q) for q in range(2, 17) for p in range(2 * q, 32 * q + 1) if math.gcd(p, q) == 1]
