"""The gather-GEMM / streaming launches of the strided and transposed convolutions in the last step of a rocprofv3 kernel
trace of `bench.py --gpus 1 --steps 20 --warmup 5` (PointPillars config, 16 frames), each named by layer and direction, with
the bytes the operation needs beside its duration; then the step's time per kernel name:
`python tools_dev/deconv_stream_calls.py <trace dir> [other trace dir]` (with two: the second one's per-kernel totals beside)."""
import collections
import csv
import glob
import os
import re
import sys

FLOOR = 5.5e12          # bytes/s a streaming kernel gets on this machine (EXPERIMENTS.md 6d: the BatchNorm apply passes)
B, H, W = 16, 248, 216
N1, N2, N3 = B * H * W, B * H * W // 4, B * H * W // 16
# layer -> (input rows, cin, output rows, cout): forward reads the input and writes the output, backward-data the reverse
LAYERS = {'D1': (N1, 64, N1, 128), 'D2': (N2, 128, N1, 128), 'D3': (N3, 256, N1, 128),
          'opener1': (4 * N1, 64, N1, 64), 'opener2': (N1, 64, N2, 128), 'opener3': (N2, 128, N3, 256)}


def last_step(d):
    f = max(glob.glob(os.path.join(d, '**', '*kernel_trace.csv'), recursive=True), key=os.path.getmtime)
    rows = list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    opt = [i for i, r in enumerate(rows) if 'multi_tensor_apply' in r['Kernel_Name']]
    # clusters of multi-tensor launches: gradient clipping's norm (after the backward) and the optimizer (after it); a step is the
    # launches from behind one optimizer cluster to the next one's end = two clusters back
    ends = [opt[i] for i in range(len(opt)) if i + 1 == len(opt) or opt[i + 1] - opt[i] > 50]
    return rows[ends[-3] + 1:ends[-1] + 1]


def us(r):
    return (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3


def short(name):
    return re.sub(r'^void ', '', name.split('(')[0])[:52]


def label(calls):
    """(layer, direction) of each call, from the kernel, its tile count and its place in the step (forward: the three stage
    openers, then D1-D3; backward: the neck first, then the stages from the last)."""
    out, seen = [], collections.Counter()
    fwd_order = ['opener1', 'opener2', 'opener3', 'opener3', 'D1', 'D2', 'D3']      # (opener3: two 128-column launches)
    wgrad_order = ['D3', 'D3', 'D2', 'D1', 'opener3', 'opener3', 'opener2']         # (256 channels: two 128-wide blocks)
    n_fwd = 0
    for r in calls:
        name, wg = r['Kernel_Name'], int(r['Workgroup_Size_X'])
        tiles = int(r['Grid_Size_X']) // wg
        m = re.search(r'deconv_stream_(fwd|bwd)_kernel<([0-9, ]+)>', name)
        if 'NP = 3' in name or re.search(r', 3>', name):
            out.append(('pillars', 'weight gradient' if 'wgrad' in name else 'backward-data'))      # first convolution on the occupied cells (pillar_conv.py, three planes)
        elif m and m.group(1) == 'fwd':
            out.append(({6696: 'D1', 1674: 'D2', 837: 'D3'}.get(tiles, '?'), 'forward'))
        elif m:
            out.append(({'1, 1, 64': 'D1', '1, 2, 128': 'D2', '2, 2, 128': 'D3'}.get(m.group(2), '?'), 'backward-data'))
        elif 'wgrad' in name:
            out.append((wgrad_order[seen['w']] if seen['w'] < len(wgrad_order) else '?', 'weight gradient'))
            seen['w'] += 1
        elif seen['w'] == 0 and n_fwd < len(fwd_order):
            out.append((fwd_order[n_fwd], 'forward'))
            n_fwd += 1
        else:
            # the neck's backward comes first: a tile count is the transposed convolution's until that one has been seen
            have = {l for l, d in out if d == 'backward-data'}
            neck, opener = {419: ('D3', 'D3'), 1674: ('D2', 'opener3'), 6696: ('D1', 'opener2')}.get(tiles, ('?', '?'))
            out.append((neck if neck not in have or tiles == 419 else opener, 'backward-data'))
    return out


def need_bytes(layer, direction, half=False):
    if layer not in LAYERS or direction == 'weight gradient':
        return None
    n_in, cin, n_out, cout = LAYERS[layer]
    d = 2 if half else 1              # a launch that produces 128 of 256 columns reads all of its input
    return 4 * (n_in * cin // d + n_out * cout) if direction == 'backward-data' else 4 * (n_in * cin + n_out * cout // d)


def main():
    step = last_step(sys.argv[1])
    pat = re.compile(r'sp_conv_x9_kernel|sp_conv_wgrad_x9_kernel|deconv_stream_')
    calls = [r for r in step if pat.search(r['Kernel_Name'])]
    print(f'{"us":>8}  {"tiles":>6}  {"layer":8} {"direction":15} {"need MB":>8} {"TB/s":>6} {"of floor":>8}  kernel')
    for r, (layer, direction) in zip(calls, label(calls)):
        t = us(r)
        half = 'sp_conv_x9' in r['Kernel_Name'] and ((layer == 'D3' and direction == 'backward-data') or (layer == 'opener3' and direction == 'forward'))
        nb = need_bytes(layer, direction, half)
        rate = f'{nb / t / 1e6:6.2f} {nb / FLOOR / (t * 1e-6):8.2f}' if nb else f'{"":6} {"":8}'
        mb = f'{nb / 1e6:8.0f}' if nb else f'{"":8}'
        print(f'{t:8.1f}  {int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]):6d}  {layer:8} {direction:15} {mb} {rate}  {short(r["Kernel_Name"])}')
    tot = collections.defaultdict(float)
    for r in step:
        tot[short(r['Kernel_Name'])] += us(r)
    other = collections.defaultdict(float)
    two = len(sys.argv) > 2
    if two:
        for r in last_step(sys.argv[2]):
            other[short(r['Kernel_Name'])] += us(r)
    print(f'\nstep: {sum(tot.values()) / 1e3:.3f} ms busy in {len(step)} launches' + (f'; other trace {sum(other.values()) / 1e3:.3f} ms' if two else ''))
    for k in sorted(set(tot) | set(other), key=lambda k: -max(tot[k], other[k])):
        if max(tot[k], other[k]) >= 20 or abs(tot[k] - other[k]) >= 30:
            print(f'{tot[k] / 1e3:9.3f} ms' + (f' {other[k] / 1e3:9.3f} ms {(tot[k] - other[k]) / 1e3:+8.3f}' if two else '') + f'  {k}')


if __name__ == '__main__':
    main()
