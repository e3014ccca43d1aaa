"""The loss phase of the last complete step of a rocprofv3 --kernel-trace directory: every kernel from the end of the last
`headconv_fwd16_kernel` to the start of the first head-backward kernel (table form of trace_region.py), the length of that
stretch, its busy time, and the launches per step of the loss kernels and fills in it.
Usage: trace_loss_phase.py <dir>"""
import collections, csv, glob, os, sys
d = sys.argv[1]
csv.field_size_limit(1 << 30)
kf = max(glob.glob(d + '/**/*_kernel_trace.csv', recursive=True), key=os.path.getmtime)
rows = list(csv.DictReader(open(kf)))
opt = sorted((int(r['Start_Timestamp']), int(r['End_Timestamp'])) for r in rows if 'FusedOptim' in r['Kernel_Name'])
ends = [en for i, (st, en) in enumerate(opt) if i + 1 == len(opt) or opt[i + 1][0] - en > 2_000_000]
t0, t1 = ends[-2], ends[-1]
ev = sorted((int(r['Start_Timestamp']), int(r['End_Timestamp']), 'q' + r.get('Queue_Id', '?') + ' s' + r.get('Stream_Id', '?'), r['Kernel_Name'])
            for r in rows if t0 <= int(r['Start_Timestamp']) < t1)
a = max(en for st, en, q, nm in ev if 'headconv_fwd16_kernel' in nm)
b = min(st for st, en, q, nm in ev if st > a and any(k in nm for k in ('headconv_wgrad16_kernel', 'head_tile_activity_kernel', 'headtail_bwd_kernel')))
busy, prev_end, count = 0, a, collections.Counter()
for st, en, q, nm in ev:
    if a <= st < b:
        gap = f'   <-- idle {(st - prev_end) / 1e3:.0f} us' if st > prev_end else ''
        print(f'{(st - t0) / 1e6:8.3f} ms {(en - st) / 1e3:7.1f} us  {q:12s} {nm[:70]}{gap}')
        busy += max(0, en - max(st, prev_end))
        prev_end = max(prev_end, en)
        count[nm.split('(')[0].replace('void ', '')[:60]] += 1
print(f'\nloss phase (end of the last headconv_fwd16_kernel -> first head-backward kernel): {(b - a) / 1e3:.1f} us, '
      f'{busy / 1e3:.1f} us of it with a kernel running, {sum(count.values())} launches')
for nm, n in sorted(count.items()):
    print(f'{n:4d} x {nm}')
