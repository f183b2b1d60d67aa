"""Model of the stream scan's trigger (modem_amd/csrc/k_stream.hip).

serial_edges   decode.cc:93-116 transcribed sample by sample: SchmittTrigger, FallingEdgeTrigger, the running maximum of the
               timing metric with its saturating age counter index_max
tiled_edges    the same as the GPU computes it: the sequence cut into tiles; each tile is a function of the incoming Schmitt state
               (state after it, falling edges in it, maximum since its last edge); a scan over those functions gives every tile its
               incoming (state, running maximum, edge count), and the tiles then emit their edges independently

Both return (t_edge, t_max, index_max) as int64 arrays.  Rate parameters: match_len, symbol_len (the correlator's, = HS), guard_len.
"""
import numpy as np

RATES = {8000: (161, 640, 160), 16000: (321, 1280, 320), 44100: (883, 3528, 882), 48000: (961, 3840, 960)}


def thresholds(match_len):
    """decode.cc:76: SchmittTrigger(value(0.17 * match_len), value(0.19 * match_len)) in fp32"""
    return np.float32(0.17 * match_len), np.float32(0.19 * match_len)


def serial_edges(timing, match_len=161, symbol_len=640, guard_len=160):
    timing = np.asarray(timing, dtype=np.float32)
    lo, hi = thresholds(match_len)
    match_del = (match_len - 1) // 2
    limit = symbol_len + guard_len + match_del
    state = False
    prev = False
    timing_max = np.float32(0)
    index_max = 0
    te, tm, im = [], [], []
    t_of_max = -1
    for t, v in enumerate(timing):
        # DSP::SchmittTrigger
        if not state and v > hi:
            state = True
        elif state and v < lo:
            state = False
        collect = state
        process = prev and not collect          # DSP::FallingEdgeTrigger
        prev = collect
        if not collect and not process:
            continue
        if timing_max < v:
            timing_max = v
            index_max = match_del
            t_of_max = t
        elif index_max < limit:
            index_max += 1
        if not process:
            continue
        te.append(t)
        tm.append(t_of_max)
        im.append(index_max)
        index_max = 0
        timing_max = np.float32(0)
    return np.array(te, np.int64), np.array(tm, np.int64), np.array(im, np.int64)


def _tile_pass(v, cls, s_in, m_in, i_in, t0, emit=None, match_del=80, limit=880):
    """one tile from the incoming (state, running maximum since the last edge, its index); -> (state out, edges, m, i, has)"""
    s, m, i = s_in, m_in, i_in
    n_e = 0
    for j in range(len(v)):
        t = t0 + j
        if cls[j] < 0 and s == 1:
            if m < v[j]:
                m, i = v[j], t
            if emit is not None:
                emit.append((t, i, min(match_del + (t - i), limit)))
            n_e += 1
            m, i = -np.inf, -1
        else:
            if m < v[j]:
                m, i = v[j], t
        if cls[j]:
            s = 1 if cls[j] > 0 else 0
    return s, n_e, m, i


def tiled_edges(timing, tile=4096, match_len=161, symbol_len=640, guard_len=160):
    timing = np.asarray(timing, dtype=np.float32)
    lo, hi = thresholds(match_len)
    match_del = (match_len - 1) // 2
    limit = symbol_len + guard_len + match_del
    n = len(timing)
    cls = np.where(timing > hi, 1, np.where(timing < lo, -1, 0)).astype(np.int8)
    ntiles = (n + tile - 1) // tile
    # 1. each tile as a function of the incoming Schmitt state: (state out, edges, maximum since its last edge, has an edge)
    fns = []
    for k in range(ntiles):
        a, b = k * tile, min(n, (k + 1) * tile)
        f = []
        for s in (0, 1):
            so, ne, m, i = _tile_pass(timing[a:b], cls[a:b], s, -np.inf, -1, a, None, match_del, limit)
            f.append((so, ne, m, i))
        fns.append(f)
    # 2. the scan over the functions: the carry entering every tile (state, running maximum, its index, edges before)
    carries = []
    s, m, i, cnt = 0, -np.inf, -1, 0
    for f in fns:
        carries.append((s, m, i, cnt))
        so, ne, fm, fi = f[s]
        if ne:
            m, i = fm, fi
        elif m < fm:
            m, i = fm, fi
        s, cnt = so, cnt + ne
    # 3. every tile emits its edges from its carry, independently of the others
    out = []
    for k in range(ntiles):
        a, b = k * tile, min(n, (k + 1) * tile)
        s, m, i, cnt = carries[k]
        emit = []
        _tile_pass(timing[a:b], cls[a:b], s, m, i, a, emit, match_del, limit)
        assert len(out) == cnt
        out.extend(emit)
    if not out:
        z = np.zeros(0, np.int64)
        return z, z.copy(), z.copy()
    e = np.array(out, np.int64)
    return e[:, 0], e[:, 1], e[:, 2]


def adversarial(n, seed, match_len=161, kind="mixed"):
    """timing sequences that stress the scan: values exactly at lo / hi, long holds between them, runs over many tiles, tied maxima,
    runs long enough to saturate index_max, a run still open at the end"""
    lo, hi = thresholds(match_len)
    rng = np.random.default_rng(seed)
    mid = np.float32((float(lo) + float(hi)) / 2)
    out = np.empty(n, np.float32)
    pos = 0
    while pos < n:
        k = rng.integers(0, 8) if kind == "mixed" else {"holds": 1, "ties": 3}.get(kind, 0)
        ln = int(rng.integers(1, 40000 if k in (1, 2) else 300))
        seg = np.empty(ln, np.float32)
        if k == 0:
            seg[:] = rng.choice(np.array([lo, hi, mid, 0.0, 2 * hi], np.float32), size=ln)
        elif k == 1:                                        # a long hold between the thresholds
            seg[:] = mid
        elif k == 2:                                        # a long run, plateaus and a late max
            seg[:] = rng.uniform(float(lo), 3 * float(hi), size=ln).astype(np.float32)
            seg[0] = 2 * hi
        elif k == 3:                                        # tied maxima
            seg[:] = rng.choice(np.array([hi * 2, hi * 2, mid, lo], np.float32), size=ln)
        elif k == 4:
            seg[:] = np.float32(0)
        elif k == 5:
            seg[:] = rng.uniform(0, 2 * float(hi), size=ln).astype(np.float32)
        elif k == 6:                                        # edges exactly at / across the thresholds
            seg[:] = np.nextafter(lo, np.float32(0)) if ln % 2 else np.nextafter(hi, np.float32(100))
        else:
            seg[:] = rng.choice(np.array([lo, np.nextafter(lo, np.float32(0)), hi, np.nextafter(hi, np.float32(100))], np.float32), size=ln)
        out[pos:pos + ln] = seg[:n - pos]
        pos += ln
    return out
