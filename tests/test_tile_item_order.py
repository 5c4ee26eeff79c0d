"""CPU: the workgroup -> (tile, item) order of the batched stage launches (csrc/common.hpp tile_item_order, handed out by the
host function drba_tile_item_order) for every tiles_x, tiles_y in 1..20 and n_items in 1..8:
  * a bijection: every (tile, item) exactly once;
  * equal to the round-4 order -- restated here -- wherever that one was banded (tile count a multiple of 8) and for one item;
  * on every XCD (workgroups b = x mod 8, ascending) the tile stays constant over runs of n_items consecutive workgroups, the
    first run possibly shorter (an XCD's range of the order may begin inside a tile's items)."""
import ctypes as C

import pytest

from drba_amd import _lib

STRIP_W = 8  # kStripW: what every kernel runs


def order(tiles_x, tiles_y, n_items, strip_w=STRIP_W):
    """[(tx, ty, item)] per workgroup id, from the library"""
    lib = _lib.load()
    tx, ty, it = C.c_int(), C.c_int(), C.c_int()
    out = []
    for b in range(tiles_x * tiles_y * n_items):
        assert lib.drba_tile_item_order(b, tiles_x, tiles_y, n_items, strip_w, C.byref(tx), C.byref(ty), C.byref(it)) == 0
        out.append((tx.value, ty.value, it.value))
    return out


# ---- the round-4 formulas, restated
def old_xcd_band(b, nblocks):
    q, r, xcd, k = nblocks >> 3, nblocks & 7, b & 7, b >> 3
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + k


def old_strip_tile(b, nblocks, tiles_x, strip_w=8):
    i = old_xcd_band(b, nblocks)
    tiles_y = nblocks // tiles_x
    rb = (tiles_y + 7) >> 3
    per_band = rb * tiles_x
    j, k = divmod(i, per_band)
    nrows = min(rb, tiles_y - j * rb)
    nfull = tiles_x // strip_w
    full = nfull * strip_w * nrows
    if k < full:
        s, r = divmod(k, strip_w * nrows)
        row, c = divmod(r, strip_w)
        col = s * strip_w + c
    else:
        wl = max(tiles_x - nfull * strip_w, 1)
        row, c = divmod(k - full, wl)
        col = nfull * strip_w + c
    return col, j * rb + row


def old_order(tiles_x, tiles_y, n_items):
    ntiles = tiles_x * tiles_y
    out = []
    for b in range(ntiles * n_items):
        if ntiles % 8 == 0 and n_items > 1:
            xcd, k = b & 7, b >> 3
            item, vb = k % n_items, (k // n_items) * 8 + xcd
        else:  # the item-major fallback
            item = b // ntiles
            vb = b - item * ntiles
        out.append(old_strip_tile(vb, ntiles, tiles_x) + (item,))
    return out


@pytest.mark.parametrize("n_items", range(1, 9))
def test_order_is_a_bijection_equals_the_banded_order_and_keeps_a_tile_on_one_xcd(n_items):
    for tiles_y in range(1, 21):
        for tiles_x in range(1, 21):
            ntiles = tiles_x * tiles_y
            got = order(tiles_x, tiles_y, n_items)
            where = f"tiles {tiles_x} x {tiles_y}, {n_items} items"
            want = {(x, y, i) for x in range(tiles_x) for y in range(tiles_y) for i in range(n_items)}
            assert len(got) == len(want) and set(got) == want, where
            if ntiles % 8 == 0 or n_items == 1:
                assert got == old_order(tiles_x, tiles_y, n_items), where
            for xcd in range(8):
                mine = got[xcd::8]  # what XCD `xcd` runs, in its order
                if not mine:
                    continue
                # the first run: the rest of a tile another XCD began
                first = next((n for n, g in enumerate(mine) if g[:2] != mine[0][:2]), len(mine))
                assert first <= n_items, where
                for s in range(first, len(mine), n_items):
                    run = mine[s:s + n_items]
                    assert len({g[:2] for g in run}) == 1, (where, xcd, s)
                    if len(run) == n_items:  # (the last run of a range may be cut by the next XCD's range)
                        assert [g[2] for g in run] == list(range(n_items)), (where, xcd, s)


@pytest.mark.parametrize("strip_w", [1, 2, 4, 8, 16])
def test_every_strip_width_walks_every_tile_once(strip_w):
    for tiles_x, tiles_y, n_items in ((1, 1, 1), (10, 3, 3), (16, 39, 8), (17, 9, 2), (5, 20, 1)):
        got = order(tiles_x, tiles_y, n_items, strip_w)
        assert sorted(got) == sorted((x, y, i) for x in range(tiles_x) for y in range(tiles_y) for i in range(n_items))
        if strip_w == 8 and n_items == 1:
            assert got == old_order(tiles_x, tiles_y, 1)


def test_rejects_what_is_not_a_launch():
    lib = _lib.load()
    v = C.c_int()
    p = C.byref(v)
    assert lib.drba_tile_item_order(0, 4, 4, 2, 8, None, p, p) == -1
    assert lib.drba_tile_item_order(32, 4, 4, 2, 8, p, p, p) == -1   # block id past the grid
    assert lib.drba_tile_item_order(-1, 4, 4, 2, 8, p, p, p) == -1
    assert lib.drba_tile_item_order(0, 0, 4, 2, 8, p, p, p) == -1
    assert lib.drba_tile_item_order(0, 4, 4, 0, 8, p, p, p) == -1
    assert lib.drba_tile_item_order(0, 4, 4, 2, 0, p, p, p) == -1
    assert lib.drba_tile_item_order(0, 1 << 16, 1 << 16, 8, 8, p, p, p) == -1  # more workgroups than an int holds
