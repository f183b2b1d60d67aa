"""Model of the segmented trigger scan behind ofdmrx_decode_streams (modem_amd/csrc/k_stream.hip).

Every recording is cut into tiles from its own position 0; a tile is the per-state function of stream_model.tiled_edges (the
kernel's StreamFn: state after it, falling edges in it, maximum since its last edge, for either incoming Schmitt state).  The tiles of
all recordings form ONE list, each recording's first tile flagged; the scan composes them with the segmented operator

    (flag_l, f_l) . (flag_r, f_r) = (flag_r, f_r)                 if flag_r      (a recording starts: nothing of the left enters)
                                    (flag_l, f_l then f_r)        otherwise

in a tree (Hillis-Steele, as block_scan_incl does), so the operator's associativity is exercised, and every tile's incoming carry is
the exclusive prefix applied to the initial carry (trigger off, no maximum, no edges).  The GPU runs one workgroup per recording, which
is this scan with the flagged elements at the workgroup boundaries.  segmented_edges returns, per recording, the (t_edge, t_max,
index_max) of stream_model.serial_edges run on that recording alone.
"""
import numpy as np

from stream_model import _tile_pass, thresholds

IDENT = tuple((s, 0, -np.inf, -1) for s in (0, 1))               # per incoming state: (state out, edges, maximum, its index)


def fn_then(l, r):
    """k_stream.hip: fn_then - the functions of two runs of tiles composed, l first"""
    out = []
    for s in (0, 1):
        q, nl, ml, il = l[s]
        so, nr, mr, ir = r[q]
        if nr:
            m, i = mr, ir
        else:
            m, i = (mr, ir) if ml < mr else (ml, il)
        out.append((so, nl + nr, m, i))
    return tuple(out)


def seg_then(l, r):
    return r if r[0] else (l[0], fn_then(l[1], r[1]))


def fn_apply(f, carry):
    """k_stream.hip: fn_apply"""
    s, m, i, cnt = carry
    so, ne, fm, fi = f[s]
    if ne or m < fm:
        m, i = fm, fi
    return so, m, i, cnt + ne


def segmented_edges(timings, tile=4096, match_len=161, symbol_len=640, guard_len=160):
    lo, hi = thresholds(match_len)
    match_del = (match_len - 1) // 2
    limit = symbol_len + guard_len + match_del
    tiles = []                                                   # (recording, a, b, values, classes)
    elems = []
    for q, timing in enumerate(timings):
        timing = np.asarray(timing, dtype=np.float32)
        cls = np.where(timing > hi, 1, np.where(timing < lo, -1, 0)).astype(np.int8)
        for a in range(0, len(timing), tile):
            b = min(len(timing), a + tile)
            f = tuple(_tile_pass(timing[a:b], cls[a:b], s, -np.inf, -1, a, None, match_del, limit) for s in (0, 1))
            tiles.append((q, a, timing[a:b], cls[a:b]))
            elems.append((a == 0, f))
    # inclusive tree scan with the segmented operator
    incl = list(elems)
    k = 1
    while k < len(incl):
        incl = [seg_then(incl[j - k], incl[j]) if j >= k else incl[j] for j in range(len(incl))]
        k <<= 1
    out = [[] for _ in timings]
    init = (0, -np.inf, -1, 0)
    for j, (q, a, v, cls) in enumerate(tiles):
        # the exclusive prefix: what the tiles before this one, back to the recording's start, make of the initial carry
        carry = init if elems[j][0] else fn_apply(incl[j - 1][1], init)
        s, m, i, cnt = carry
        assert cnt == len(out[q])
        _tile_pass(v, cls, s, m, i, a, out[q], match_del, limit)
    res = []
    for e in out:
        a = np.array(e, np.int64).reshape(-1, 3)
        res.append((a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy()))
    return res


def leak_pair(match_len=161, n0=4097, n1=300):
    """two sequences a leaked trigger state would betray: the first ends above hi (its trigger is on at the end), the second starts
    between lo and hi and then falls below lo - with the first one's state entering it, that is a falling edge; alone, it is none"""
    lo, hi = thresholds(match_len)
    mid = np.float32((float(lo) + float(hi)) / 2)
    a = np.zeros(n0, np.float32)
    a[-50:] = 2 * hi
    b = np.full(n1, mid, np.float32)
    b[n1 // 2:] = lo / 2
    return a, b
