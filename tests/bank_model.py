"""Model of the live feed bank's trigger scan (modem_amd/csrc/api_bank.cpp): the tile model of feed_model.py for C
channels whose pushes interleave.  ONE driver works a push for all channels, as the device does: the tiles every channel completed
are packed into one per-tile array (channel c's at tile_at[c] .. tile_at[c + 1]), a SEGMENTED scan composes each channel's stretch of
that array alone - from that channel's carry-in, leaving that channel's carry-out; a channel without tiles keeps its carry - and the
tiles then emit their edges into their channel's list, counted from 0 per channel per push.  This is the written statement of what
k_bank_fn_scan and the WindowBatch forms of k_stream_tile must do: nothing of a channel is ever composed with its neighbour's."""
import numpy as np

from stream_model import _tile_pass, thresholds


class BankScan:
    def __init__(self, n_channels, tile=4096, match_len=161, symbol_len=640, guard_len=160):
        self.C, self.tile, self.match_len = n_channels, tile, match_len
        self.match_del = (match_len - 1) // 2
        self.limit = symbol_len + guard_len + self.match_del
        self.lo, self.hi = thresholds(match_len)
        self.buf = [np.zeros(0, np.float32) for _ in range(n_channels)]   # the windows: timing values from base[c] on
        self.base = [0] * n_channels
        self.fed = [0] * n_channels
        self.scanned = [0] * n_channels          # multiples of the tile until the channel ends
        self.carry = [(0, -np.inf, -1)] * n_channels
        self.ended = [False] * n_channels
        self.edges = [[] for _ in range(n_channels)]

    def _step(self, t_end):
        """one pass over the tiles [scanned[c] / tile, t_end[c]) of every channel"""
        tiles, tile_at = [], [0]
        for c in range(self.C):                  # the packed per-tile array
            for k in range(self.scanned[c] // self.tile, t_end[c]):
                a, b = k * self.tile, min(self.fed[c], (k + 1) * self.tile)
                v = self.buf[c][a - self.base[c]:b - self.base[c]]
                cls = np.where(v > self.hi, 1, np.where(v < self.lo, -1, 0)).astype(np.int8)
                fn = [_tile_pass(v, cls, s, -np.inf, -1, a, None, self.match_del, self.limit) for s in (0, 1)]
                tiles.append((a, v, cls, fn))
            tile_at.append(len(tiles))
        carries = [None] * len(tiles)
        counts = [0] * self.C
        carry_out = list(self.carry)             # (a channel without tiles keeps its carry)
        for c in range(self.C):                  # the segmented scan: one segment per channel, from its own carry-in
            s, m, i = self.carry[c]
            count = 0
            for t in range(tile_at[c], tile_at[c + 1]):
                carries[t] = (s, m, i, count)
                so, ne, fm, fi = tiles[t][3][s]
                if ne or m < fm:
                    m, i = fm, fi
                s, count = so, count + ne
            if tile_at[c + 1] > tile_at[c]:
                carry_out[c] = (s, m, i)
            counts[c] = count
        out = [[None] * n for n in counts]       # edges [channels][cap]
        for c in range(self.C):
            for t in range(tile_at[c], tile_at[c + 1]):
                a, v, cls, fn = tiles[t]
                cs, cm, ci, cc = carries[t]
                emit = []
                _tile_pass(v, cls, cs, cm, ci, a, emit, self.match_del, self.limit)
                out[c][cc:cc + len(emit)] = emit
        for c in range(self.C):
            assert all(e is not None for e in out[c])
            self.edges[c] += out[c]
        self.carry = carry_out

    def push(self, blocks, ends=None):
        """blocks[c]: channel c's new timing values (None / empty: none); ends[c]: the channel is over after them"""
        t_end = []
        for c in range(self.C):
            blk = np.zeros(0, np.float32) if blocks[c] is None else np.asarray(blocks[c], np.float32)
            assert not (self.ended[c] and len(blk))
            self.buf[c] = np.concatenate([self.buf[c], blk])
            self.fed[c] += len(blk)
            if self.ended[c]:
                t_end.append(self.scanned[c] // self.tile)      # no tiles
            elif ends is not None and ends[c]:
                t_end.append((self.fed[c] + self.tile - 1) // self.tile)
            else:
                t_end.append(self.fed[c] // self.tile)
        t_end = [max(t, s // self.tile) for t, s in zip(t_end, self.scanned)]
        self._step(t_end)
        for c in range(self.C):
            if self.ended[c]:
                continue
            if ends is not None and ends[c]:
                self.scanned[c], self.ended[c] = self.fed[c], True
            else:
                self.scanned[c] = t_end[c] * self.tile
                drop = self.scanned[c] - self.base[c]            # the model's window keeps nothing behind the frontier
                self.buf[c], self.base[c] = self.buf[c][drop:], self.scanned[c]

    def end(self):
        self.push([None] * self.C, ends=[True] * self.C)
        res = []
        for c in range(self.C):
            if not self.edges[c]:
                z = np.zeros(0, np.int64)
                res.append((z, z.copy(), z.copy()))
                continue
            e = np.array(self.edges[c], np.int64)
            res.append((e[:, 0], e[:, 1], e[:, 2]))
        return res


def bank_edges(timings, rounds, ends=None, **kw):
    """timings[c] pushed by rounds[r][c] values per round (ends: {round: channels that end with it}) -> per channel (g, t_max, index_max)"""
    b = BankScan(len(timings), **kw)
    at = [0] * len(timings)
    for r, lens in enumerate(rounds):
        blocks = [timings[c][at[c]:at[c] + n] for c, n in enumerate(lens)]
        e = None if not ends or r not in ends else [c in ends[r] for c in range(len(timings))]
        b.push(blocks, ends=e)
        at = [a + n for a, n in zip(at, lens)]
    return b.end()
