"""Timeline of the last bench step in a rocprofv3 kernel_trace.csv: per 20-ms bin, the number of
streams with a kernel in flight, the share of the bin covered by GPU-filling kernels (>= 1024
workgroups) and by the latency-bound ones (k_dfs_pool, k_small_loop), and for each of those two the share of the
tile phase with a launch in flight; then how long the fill streams are held in the tile phase: per kind of borrow
(a worker thread's run of kernels on a fill stream between two fill_release calls) the span from its first kernel's
start to its last kernel's end against the sum of its kernels' durations, and what k_single_tail and the spectra
kernel for segments above 64 pixels hold of the spans.  python tools/timeline.py TRACE.csv"""
import csv, sys, collections
rows = []
meta = {}         # (start, end, name) of a row -> (stream, launching thread), for the fill-stream hold
missing = []
with open(sys.argv[1]) as fh:
    rd = csv.DictReader(fh)
    missing = [c for c in ('Stream_Id', 'Thread_Id') if c not in (rd.fieldnames or [])]
    for r in rd:
        g = int(r.get('Grid_Size_X', 0) or 0) * max(int(r.get('Grid_Size_Y', 1) or 1), 1)
        w = max(int(r.get('Workgroup_Size_X', 1) or 1) * max(int(r.get('Workgroup_Size_Y', 1) or 1), 1), 1)
        rows.append((int(r['Start_Timestamp']), int(r['End_Timestamp']), r['Kernel_Name'], r.get('Queue_Id', '0'), g // w))
        meta[(rows[-1][0], rows[-1][1], rows[-1][2])] = (r.get('Stream_Id', r.get('Queue_Id', '0')), r.get('Thread_Id', '0'))
rows.sort()
# the last step starts at the last k_subsample / first k_fit after a gap: take the last k_synthimg-free span
fits = [s for s, e, n, q, b in rows if n.startswith('k_subsample')]
t0 = fits[-1] if fits else rows[0][0]
rows = [r for r in rows if r[0] >= t0]
t1 = max(r[1] for r in rows)
BIN = 20e6
nb = int((t1 - t0) / BIN) + 1
fill = [0.0] * nb; lat = [0.0] * nb; qs = [set() for _ in range(nb)]
def cover(iv, lo, hi):
    iv = sorted((max(s, lo), min(e, hi)) for s, e in iv if e > lo and s < hi)
    tot = 0; cur = None
    for s, e in iv:
        if cur is None or s > cur[1]:
            if cur: tot += cur[1] - cur[0]
            cur = [s, e]
        else: cur[1] = max(cur[1], e)
    if cur: tot += cur[1] - cur[0]
    return tot
F = [(s, e) for s, e, n, q, b in rows if b >= 1024 and not n.startswith(('k_dfs_split', 'k_dfs_pool', 'k_small_loop'))]
Lt = [(s, e) for s, e, n, q, b in rows if n.startswith(('k_dfs_split', 'k_dfs_pool', 'k_small_loop'))]
print('step span %.1f ms; sum of GPU-filling kernel durations %.1f ms; union %.1f ms' % (
    (t1 - t0) / 1e6, sum(e - s for s, e in F) / 1e6, cover(F, t0, t1) / 1e6))
# the tile phase (first k_ccl_local to the end of the last latency-bound kernel) and what the two walker classes
# hold of it: launches, the share of the phase with a launch in flight (union), time and workgroups per launch
ccl = [s for s, e, n, q, b in rows if n.startswith('k_ccl_local')]
if ccl and Lt:
    p0, p1 = min(ccl), max(e for s, e in Lt)
    print('tile phase %.1f ms' % ((p1 - p0) / 1e6))
    for cls in ('k_dfs_pool', 'k_small_loop'):
        K = [(s, e, b) for s, e, n, q, b in rows if n.startswith(cls)]
        if K:
            d = sorted((e - s) / 1e6 for s, e, b in K)
            print('   %-13s %4d launches  in flight %.2f of the tile phase  ms per launch mean %.2f median %.2f max %.2f  '
                  'workgroups mean %.1f most %d' % (cls, len(K), cover([(s, e) for s, e, b in K], p0, p1) / (p1 - p0),
                                                    sum(d) / len(d), d[len(d) // 2], d[-1],
                                                    sum(b for s, e, b in K) / len(K), max(b for s, e, b in K)))
    print('   either        in flight %.2f of the tile phase' % (cover(Lt, p0, p1) / (p1 - p0)))
# Fill-stream hold.  The fill streams are those that run k_ccl_local.  Borrows are told apart by the launching thread
# (two fill streams on one hardware queue are not always told apart in the trace's stream column): a thread's kernels
# on the fill streams, in time order, open a new borrow at the first kernel of a phase -- k_ccl_local (A: local
# labels up to the replay's order), k_scan_local<SeedFn> (B: seed scan to the last kernel before the pass loop),
# k_scan_local<EmptyFn> not preceded by k_single_tail (C: the relabel after the pass loop), a run of k_assign -- and at
# any other kernel after a pause of the thread above 5 ms.
def short(n):
    n = n.split('(')[0]
    return n[5:] if n.startswith('void ') else n
fstreams = {meta[(s, e, n)][0] for s, e, n, q, b in rows if n.startswith('k_ccl_local')}
if ccl and Lt and fstreams:
    per = collections.defaultdict(list)
    for s, e, n, q, b in rows:
        st, th = meta[(s, e, n)]
        if st in fstreams and e > p0 and s < p1: per[th].append((s, e, short(n)))
    borrows = []                     # [kind, start, end, sum of durations, single_tail, spectra_big, kernels]
    for th, ks in per.items():
        cur = None; prev = None
        for s, e, n in ks:
            kind = None
            if n.startswith('k_ccl_local'): kind = 'A clump'
            elif n.startswith('k_scan_local<SeedFn>'): kind = 'B to the pass loop'
            elif n.startswith('k_scan_local<EmptyFn>') and not (prev or '').startswith('k_single_tail'): kind = 'C relabel'
            elif n.startswith('k_assign') and not (prev or '').startswith('k_assign'): kind = 'assign'
            elif cur is None or s - cur[2] > 5e6: kind = 'other'
            if kind: cur = [kind, s, e, 0, 0, 0, 0]; borrows.append(cur)
            cur[2] = max(cur[2], e); cur[3] += e - s; cur[6] += 1
            if n.startswith('k_single_tail'): cur[4] += e - s
            if n.startswith('k_spectra_big'): cur[5] += e - s
            prev = n
    if missing:
        print('NOTE: the trace has no %s column: %s; the hold figures below are not to be trusted' % (
            ' / '.join(missing), 'streams are taken from Queue_Id' if 'Stream_Id' in missing and len(missing) == 1 else
            'borrows of different threads cannot be told apart'))
    print('fill streams: %d (stream ids %s), offered %.1f ms of stream time in the tile phase' % (
        len(fstreams), ' '.join(sorted(fstreams)), len(fstreams) * (p1 - p0) / 1e6))
    tot = [0, 0, 0, 0]
    for kind in sorted({b[0] for b in borrows}):
        B = [b for b in borrows if b[0] == kind]
        span = sum(b[2] - b[1] for b in B); ksum = sum(b[3] for b in B)
        tot[0] += span; tot[1] += ksum; tot[2] += sum(b[4] for b in B); tot[3] += sum(b[5] for b in B)
        print('   %-20s %4d borrows  %5.1f kernels each  span mean %7.3f ms  sum %7.1f ms   kernels mean %7.3f ms  sum %7.1f ms' % (
            kind, len(B), sum(b[6] for b in B) / len(B), span / len(B) / 1e6, span / 1e6, ksum / len(B) / 1e6, ksum / 1e6))
    ntile = max(sum(1 for b in borrows if b[0].startswith('B')), 1)
    print('   all borrows: held %.1f ms (%.2f of the offered), kernels %.1f ms; per tile held %.3f ms, kernels %.3f ms' % (
        tot[0] / 1e6, tot[0] / (len(fstreams) * (p1 - p0)), tot[1] / 1e6, tot[0] / ntile / 1e6, tot[1] / ntile / 1e6))
    print('   of the held time: k_single_tail %.1f ms (%.3f), spectra above 64 pixels %.1f ms (%.3f)' % (
        tot[2] / 1e6, tot[2] / max(tot[0], 1), tot[3] / 1e6, tot[3] / max(tot[0], 1)))
for i in range(nb):
    lo, hi = t0 + i * BIN, min(t0 + (i + 1) * BIN, t1)
    nq = len({q for s, e, n, q, b in rows if e > lo and s < hi})
    nl = sum(1 for s, e in Lt if e > lo and s < hi)
    print('%5.0f ms  queues %2d  latency-bound kernels in flight %2d  filling-union %.2f  sum-of-filling %.2f' % (
        (lo - t0) / 1e6, nq, nl, cover(F, lo, hi) / (hi - lo), sum(min(e, hi) - max(s, lo) for s, e in F if e > lo and s < hi) / (hi - lo)))
# what runs at the very end of the step (after the last latency-bound kernel has finished)
lastwalk = max([e for s, e in Lt] or [t0])
tail = collections.defaultdict(lambda: [0, 0.0])
for s, e, n, q, b in rows:
    if s >= lastwalk:
        k = tail[n.split('(')[0][:44]]
        k[0] += 1; k[1] += (e - s) / 1e6
print('after the last walker (%.1f ms before the end):' % ((t1 - lastwalk) / 1e6))
for n, (c, ms) in sorted(tail.items(), key=lambda kv: -kv[1][1])[:12]:
    print('   %-46s %4d launches %8.2f ms' % (n, c, ms))
