"""Cluster images that drive the depth-first cut replay of the clump stage (pyshepseg_amd/csrc/clump.h)
through every step of its walker, and a host model of the reference's loop that counts what each walk does.

Importable without a GPU.  make(name) is an int32 cluster image (0 = null); padded() moves it off the raster
edges and off word alignment; replay_census() replays the reference's size-capped depth-first growth in plain
Python and returns the labels, the next id and a census of the walk; bitmap_words() is the size of the visited
bitmap the device walker needs per cut component (dfs_bitmap_words of clump.h).

What the walks reach, 4-connected, as replay_census() counts it (a mask is the set of unvisited member neighbours
a popped pixel pushes: bit 0 left, 1 up, 2 right, 3 down; a streak is a run of consecutive pops of one piece with
the same mask; "dead" is mask 0).  tests/test_clump_shapes_host.py asserts the bounds that follow from it.

  shape          px cut  capped  cap in   one-px in  stack   dead run   streaks longer than 62 of masks
                 comps   pieces  streak   cut comp   depth   max / >64  1 / 2 / 3 / 4 / 6 / 8 / 9 / 12 / 14
  percolation        1       4       0        382    1917    40 / 0    0 / 0 / 0 / 0 / 0 / 0 / 0 / 0 / 0
  percolation8       0       0       0          0      40    19 / 0    0 / 0 / 0 / 0 / 0 / 0 / 0 / 0 / 0
  serp_h1            1       2       2          0       2     1 / 0    65 / 0 / 0 / 196 / 0 / 0 / 0 / 0 / 0
  serp_v1            1       2       2          0       2     1 / 0    0 / 65 / 0 / 0 / 0 / 195 / 0 / 0 / 0
  strips_v2          1       1       1          0     357   219 / 70   0 / 0 / 0 / 0 / 0 / 70 / 70 / 0 / 0
  strips_h2          1       3       3          0     220   219 / 70   0 / 0 / 0 / 70 / 0 / 0 / 0 / 73 / 0
  strips_h2_low      1       3       3          0     229   229 / 71   0 / 0 / 0 / 74 / 74 / 0 / 0 / 0 / 0
  strips_h3_mid      1       3       3          0     457   456 / 56   3 / 0 / 0 / 54 / 0 / 0 / 0 / 4 / 55
  strips_v2_up       1       1       1          0     528   228 / 73   0 / 0 / 21 / 0 / 0 / 74 / 54 / 0 / 0
  lattice3           1       2       1          1    2039  1851 / 1    0 / 0 / 0 / 0 / 0 / 0 / 0 / 0 / 0
  comb_up            1       1       1          0     130     1 / 0    0 / 48 / 0 / 0 / 0 / 213 / 0 / 0 / 0
  comb_down          1       1       1          0     131     1 / 0    0 / 0 / 0 / 0 / 0 / 261 / 0 / 0 / 0
  rings              1       2       2          0      72     2 / 0    59 / 53 / 0 / 155 / 0 / 125 / 0 / 0 / 0
  rect_widths        5       9       9          0    4986   733 / 8    0 / 4 / 96 / 0 / 0 / 4 / 112 / 4 / 0
(A streak the cap cuts short counts with the length it had.)  4-connected, `percolation8` holds no component above
432 pixels; 8-connected it holds one of 47757 pixels, cut into 3 capped pieces and the rest.  `many_big` (289 components of 10100 pixels, more than the 256 workgroups the walk launches
at most) is left out of the model: the replay in Python takes seconds there."""
import numpy as np

CAP = 10000                  # pixels added to a piece after which the reference stops growing it
BIG = CAP + 2                # the smallest component the cap can cut

MODEL_SHAPES = ('percolation', 'percolation8', 'serp_h1', 'serp_v1', 'strips_v2', 'strips_h2', 'strips_h2_low',
                'strips_h3_mid', 'strips_v2_up', 'lattice3', 'comb_up', 'comb_down', 'rings', 'rect_widths')
SHAPES = MODEL_SHAPES + ('many_big',)
RUNNABLE = (1, 4, 12, 6, 14, 8, 9, 2, 3)          # the masks whose streaks the walker takes in one go


def _percolation(eight):
    rs = np.random.RandomState(7)
    a = rs.rand(300, 330) < 0.66
    b = rs.rand(300, 330) < 0.5                   # (the draws continue: one generator for both)
    return (b if eight else a).astype(np.int32)


def _serp_h1():
    cl = np.ones((260, 200), dtype=np.int32)
    cl[1::2, :] = 2
    cl[1::4, -1] = 1
    cl[3::4, 0] = 1
    return cl


def _strips_v2():
    cl = np.full((220, 210), 2, dtype=np.int32)
    for c in range(0, 210, 3):
        cl[:, c:c + 2] = 1
    cl[0, :] = 1
    return cl


def _strips_h2_low():
    cl = np.full((222, 230), 2, dtype=np.int32)
    for r in range(0, 220, 3):
        cl[r:r + 2, 2:] = 1
        cl[r + 1, 1] = 1
    cl[:, 0] = 1
    return cl


def _strips_h3_mid():
    cl = np.full((221, 230), 2, dtype=np.int32)
    for r in range(0, 220, 4):
        cl[r:r + 3, 2:] = 1
        cl[r + 1, 1] = 1
    cl[:, 0] = 1
    return cl


def _strips_v2_up():
    cl = np.full((230, 222), 2, dtype=np.int32)
    for c in range(0, 220, 3):
        cl[:-2, c:c + 2] = 1
        cl[-2, c + 1] = 1
    cl[-1, :] = 1
    return cl


def _lattice3():
    cl = np.full((230, 230), 2, dtype=np.int32)
    cl[::3, :] = 1
    cl[:, ::3] = 1
    return cl


def _comb(up):
    cl = np.full((200, 260), 2, dtype=np.int32)
    cl[:, ::2] = 1
    cl[-1 if up else 0, :] = 1
    return cl


def _rings():
    """one-pixel square rings at distances 0, 2, 4 ... from the edge; ring k is linked to ring k + 2 by one
    pixel, in turn in the middle of the top and of the bottom side"""
    n = 241
    cl = np.full((n, n), 2, dtype=np.int32)
    for k in range(0, n // 2 + 1, 2):
        cl[k, k:n - k] = 1
        cl[n - 1 - k, k:n - k] = 1
        cl[k:n - k, k] = 1
        cl[k:n - k, n - 1 - k] = 1
        if k + 2 <= n // 2:
            cl[k + 1 if k % 4 == 0 else n - 2 - k, n // 2] = 1
    return cl


def _rect_widths():
    cl = np.full((345, 284), 9, dtype=np.int32)
    c = 0
    for v, (w, h) in enumerate(((30, 340), (31, 345), (62, 340), (63, 345), (94, 340)), start=1):
        cl[:h, c:c + w] = v
        c += w + 1
    assert c - 1 == 284
    return cl


def _many_big():
    (i, j) = np.mgrid[0:17, 0:17]
    return np.kron((i * 17 + j) % 7 + 1, np.ones((101, 100), dtype=np.int64)).astype(np.int32)


_MAKERS = {
    'percolation': lambda: _percolation(False),
    'percolation8': lambda: _percolation(True),
    'serp_h1': _serp_h1,
    'serp_v1': lambda: _serp_h1().T,
    'strips_v2': _strips_v2,
    'strips_h2': lambda: _strips_v2().T,
    'strips_h2_low': _strips_h2_low,
    'strips_h3_mid': _strips_h3_mid,
    'strips_v2_up': _strips_v2_up,
    'lattice3': _lattice3,
    'comb_up': lambda: _comb(True),
    'comb_down': lambda: _comb(False),
    'rings': _rings,
    'rect_widths': _rect_widths,
    'many_big': _many_big,
}
_made = {}


def make(name):
    """the int32 cluster image of a shape (0 = null); built once, handed out read-only"""
    if name not in _made:
        cl = np.ascontiguousarray(_MAKERS[name](), dtype=np.int32)
        cl.setflags(write=False)
        _made[name] = cl
    return _made[name]


def padded(cl):
    """the same image inside a null margin (1 row on top, 33 columns left, 2 right, 1 row at the bottom): no
    component touches a raster edge, and the label addresses of a row shift off word alignment"""
    out = np.zeros((cl.shape[0] + 2, cl.shape[1] + 35), dtype=np.int32)
    out[1:-1, 33:-2] = cl
    return out


def _streak_end(cen, m, run):
    if run > cen['longest'][m]:
        cen['longest'][m] = run
    if run > 62:
        cen['over62'][m] += 1
    if m == 0 and run > 64:
        cen['dead_over64'] += 1


def replay_census(cl, four, cap=CAP):
    """The reference's clump loop on `cl` (ids from 1): (labels uint32, next id, census).

    A raster scan seeds a piece at every pixel that is neither null nor labelled.  The piece grows from an explicit
    stack: pop the last entry, look at its 3 x 3 window column by column (column offset outer, row offset inner;
    4-connected: left, up, down, right), label and push every neighbour of the seed's value that has no label
    yet.  The growth stops when the stack is empty or once `cap` pixels were added; what is still on the stack
    keeps its label.  cap=None grows without limit: the true components.

    census, 4-connected: 'pops'[m], 'longest'[m], 'over62'[m] per mask m (longest streak, streaks longer than 62;
    m = 0: runs of dead pops), 'dead_over64', 'depth' (largest number of stack entries), 'capped' (pieces that
    ended on the cap), 'capped_in_streak' (... while the last two pops or more had the same mask), 'single_seeds'
    (the (row, col) of every one-pixel piece).  8-connected: 'pops' per number of neighbours pushed (0 .. 8),
    'longest'[0], 'dead_over64', 'depth', 'capped', 'single_seeds'."""
    (nr, nc) = cl.shape
    pitch = nc + 2
    img = np.zeros((nr + 2, pitch), dtype=np.int64)
    img[1:-1, 1:-1] = cl
    val = img.ravel().tolist()
    out = [0] * len(val)
    if four:
        nbrs = ((-1, 1), (-pitch, 2), (pitch, 8), (1, 4))
    else:
        nbrs = tuple((dx + dy * pitch, 1 << i) for i, (dx, dy) in enumerate(
            (dx, dy) for dx in (-1, 0, 1) for dy in (-1, 0, 1) if (dx, dy) != (0, 0)))
    nmask = 16 if four else 256
    cen = {'pops': [0] * nmask, 'longest': [0] * nmask, 'over62': [0] * nmask, 'dead_over64': 0, 'depth': 0,
           'capped': 0, 'capped_in_streak': 0, 'single_seeds': []}
    pops = cen['pops']
    limit = cap if cap is not None else len(val)
    nid = 1
    depth = 0
    for r in range(1, nr + 1):
        for seed in range(r * pitch + 1, r * pitch + 1 + nc):
            v = val[seed]
            if v == 0 or out[seed]:
                continue
            out[seed] = nid
            stack = [seed]
            cnt = 0
            prev = -1
            run = 0
            while stack and cnt < limit:
                p = stack.pop()
                m = 0
                for (off, bit) in nbrs:
                    q = p + off
                    if val[q] == v and not out[q]:
                        out[q] = nid
                        stack.append(q)
                        cnt += 1
                        m |= bit
                pops[m] += 1
                if m == prev:
                    run += 1
                else:
                    if prev >= 0:
                        _streak_end(cen, prev, run)
                    prev = m
                    run = 1
                if len(stack) > depth:
                    depth = len(stack)
            _streak_end(cen, prev, run)
            if cnt >= limit:
                cen['capped'] += 1
                if run >= 2:
                    cen['capped_in_streak'] += 1
            if cnt == 0:
                cen['single_seeds'].append((r - 1, seed - r * pitch - 1))
            nid += 1
    cen['depth'] = depth
    if not four:                                   # per number of neighbours pushed
        by = [0] * 9
        for m, n in enumerate(pops):
            by[bin(m).count('1')] += n
        cen = {'pops': by, 'longest': [cen['longest'][0]], 'dead_over64': cen['dead_over64'], 'depth': depth,
               'capped': cen['capped'], 'single_seeds': cen['single_seeds']}
    lab = np.array(out, dtype=np.uint32).reshape(nr + 2, pitch)[1:-1, 1:-1]
    return np.ascontiguousarray(lab), nid, cen


def components(cl, four):
    """(labels, sizes) of the true components: the replay without a cap"""
    lab, _nxt, _cen = replay_census(cl, four, cap=None)
    return lab, np.bincount(lab.ravel())


def cut_components(cl, four):
    """per true component of >= 10002 pixels, in raster order of their first pixels:
    (first row, last row, first column, last column, size)"""
    lab, sizes = components(cl, four)
    out = []
    for i in np.flatnonzero(sizes >= BIG):
        if i == 0:
            continue
        m = lab == i
        rows = np.flatnonzero(m.any(axis=1))
        cols = np.flatnonzero(m.any(axis=0))
        out.append((int(rows[0]), int(rows[-1]), int(cols[0]), int(cols[-1]), int(sizes[i])))
    return out


def bitmap_words(cl, four):
    """words of the walker's visited bitmap for every component the cap can cut: its bounding box with a one-bit
    border, rows of whole 32-bit words and at least two of them"""
    return [(r1 - r0 + 3) * max(2, (c1 - c0 + 3 + 31) // 32) for (r0, r1, c0, c1, _n) in cut_components(cl, four)]


def singles_in_cut(cl, four, cen):
    """how many of the census' one-pixel pieces lie in a component of >= 10002 pixels"""
    lab, sizes = components(cl, four)
    return sum(1 for (r, c) in cen['single_seeds'] if sizes[lab[r, c]] >= BIG)


def census_row(name):
    """one line of the table in this module's docstring"""
    cl = make(name)
    _lab, _nxt, c = replay_census(cl, True)
    return '  %-14s %5d  %6d  %6d   %8d  %6d  %4d / %-4d %s' % (
        name, len(cut_components(cl, True)), c['capped'], c['capped_in_streak'], singles_in_cut(cl, True, c),
        c['depth'], c['longest'][0], c['dead_over64'], ' / '.join('%d' % c['over62'][m] for m in (1, 2, 3, 4, 6, 8, 9, 12, 14)))


if __name__ == '__main__':                         # prints the table above
    for nm in MODEL_SHAPES:
        print(census_row(nm))
    print(max(n for (*_b, n) in cut_components(make('percolation8'), False)))
