"""Model of the live feed's trigger scan (modem_amd/csrc/api_bank.cpp with one channel): the tile model of stream_model.py run push by
push.  A push scans the tiles it has completed - tiles stay on absolute multiples of the tile length - from the carry the last push
left (Schmitt state, running maximum since the last falling edge and its index; the edge count starts at 0 in every push), and
leaves the carry for the next; end() scans the last partial tile."""
import numpy as np

from stream_model import _tile_pass, thresholds


class FeedScan:
    def __init__(self, tile=4096, match_len=161, symbol_len=640, guard_len=160):
        self.tile, self.match_len = tile, match_len
        self.match_del = (match_len - 1) // 2
        self.limit = symbol_len + guard_len + self.match_del
        self.lo, self.hi = thresholds(match_len)
        self.buf = np.zeros(0, np.float32)      # the window: timing values from `base` on
        self.base = 0
        self.fed = 0
        self.scanned = 0                        # a multiple of the tile until end()
        self.carry = (0, -np.inf, -1)           # what enters the next tile
        self.edges = []

    def _scan(self, t_end):
        """tiles [scanned / tile, t_end): each as a function of the incoming state, the scan of those, then the edges"""
        tiles = []
        for k in range(self.scanned // self.tile, t_end):
            a, b = k * self.tile, min(self.fed, (k + 1) * self.tile)
            v = self.buf[a - self.base:b - self.base]
            cls = np.where(v > self.hi, 1, np.where(v < self.lo, -1, 0)).astype(np.int8)
            fn = [_tile_pass(v, cls, s, -np.inf, -1, a, None, self.match_del, self.limit) for s in (0, 1)]
            tiles.append((a, v, cls, fn))
        s, m, i = self.carry
        count = 0                               # edges of this push before the tile
        carries = []
        for a, v, cls, fn in tiles:
            carries.append((s, m, i, count))
            so, ne, fm, fi = fn[s]
            if ne or m < fm:
                m, i = fm, fi
            s, count = so, count + ne
        out = [None] * count
        for (a, v, cls, fn), (cs, cm, ci, cc) in zip(tiles, carries):
            emit = []
            _tile_pass(v, cls, cs, cm, ci, a, emit, self.match_del, self.limit)
            out[cc:cc + len(emit)] = emit
        assert all(e is not None for e in out)
        self.edges += out
        self.carry = (s, m, i)

    def push(self, timing):
        timing = np.asarray(timing, np.float32)
        self.buf = np.concatenate([self.buf, timing])
        self.fed += len(timing)
        t_end = self.fed // self.tile
        self._scan(t_end)
        self.scanned = t_end * self.tile
        drop = self.scanned - self.base         # the model's window keeps nothing behind the frontier
        self.buf, self.base = self.buf[drop:], self.scanned

    def end(self):
        self._scan((self.fed + self.tile - 1) // self.tile)
        self.scanned = self.fed
        if not self.edges:
            z = np.zeros(0, np.int64)
            return z, z.copy(), z.copy()
        e = np.array(self.edges, np.int64)
        return e[:, 0], e[:, 1], e[:, 2]


def feed_edges(timing, cuts, **kw):
    f = FeedScan(**kw)
    pos = [0] + [int(c) for c in cuts] + [len(timing)]
    for a, b in zip(pos[:-1], pos[1:]):
        f.push(timing[a:b])
    return f.end()
