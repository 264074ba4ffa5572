"""Per-launch summary of one pipeline chunk from a rocprofv3 kernel trace of the benchmark.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o bench -- \
        python bench.py --gpus 1 --steps 2 --warmup 1 --cpu-seconds 0 --no-secondary
    python tools/chunk_trace_summary.py DIR/bench_kernel_trace.csv [OUT.json]

Every launch of a full chunk (8192 queries of p2s_max) gets its layer name from its kernel, its grid and its place behind the
two chain launches: SF1, SF2, SF3, fold behind the STN pass, D1, D2, D3, tail behind the main pass, kNN and gather ahead of
both.  Per layer over all full chunks of the trace: median / mean / standard deviation of the duration, the median idle gap to
the next launch of the same queue, grid, registers and LDS; for the FC layers the fraction of the fp32 MFMA peak
(2 M N K Z / duration / 157.3 TFLOP/s)."""
import csv
import json
import statistics
import sys

PEAK = 157.3e12
CHUNK = 8192
# layer: (N, K, Z)
FC = {'SF1': (512, 1024, 2), 'SF2': (256, 512, 2), 'SF3': (4096, 256, 2), 'D1': (512, 1024, 2), 'D2': (256, 1024, 1),
      'D3': (128, 256, 1)}
ORDER = ('kNN', 'gather', 'chain_stn', 'SF1', 'SF2', 'SF3', 'fold', 'chain_main', 'D1', 'D2', 'D3', 'tail')


def short(name):
    for key, tag in (('p2s_chain_save_kernel', 'chain_stn'), ('p2s_chain_reuse_kernel', 'chain_main'), ('p2s_chain_kernel', 'chain'),
                     ('p2s_gemm_kernel', 'gemm'), ('p2s_fold_kernel', 'fold'), ('p2s_knn_kernel', 'kNN'),
                     ('p2s_gather_kernel', 'gather'), ('p2s_decoder_tail_kernel', 'tail')):
        if key in name:
            return tag
    return None


def load(path):
    rows = []
    with open(path, newline='') as f:
        for r in csv.DictReader(f):
            tag = short(r['Kernel_Name'])
            rows.append({'tag': tag, 'name': r['Kernel_Name'], 'queue': (r['Agent_Id'], r['Queue_Id']),
                         'start': int(r['Start_Timestamp']), 'end': int(r['End_Timestamp']),
                         'grid': (int(r['Grid_Size_X']), int(r['Grid_Size_Y']), int(r['Grid_Size_Z'])),
                         'wg': int(r['Workgroup_Size_X']), 'vgpr': int(r['VGPR_Count']), 'agpr': int(r['Accum_VGPR_Count']),
                         'sgpr': int(r['SGPR_Count']), 'lds': int(r['LDS_Block_Size']), 'scratch': int(r['Scratch_Size'])})
    rows.sort(key=lambda r: r['start'])
    return rows


def label(rows):
    """names the FC launches by their place; marks the launches of full chunks"""
    by_queue = {}
    for r in rows:
        by_queue.setdefault(r['queue'], []).append(r)
    for q in by_queue.values():
        for a, b in zip(q, q[1:]):
            a['gap'] = b['start'] - a['end']
            a['next'] = b['tag'] or b['name'].split('(')[0][-40:]
    last, n = None, 0
    for r in rows:
        if r['tag'] in ('chain_stn', 'chain_main', 'chain'):
            last, n = r['tag'], 0
        elif r['tag'] == 'gemm':
            names = ('SF1', 'SF2', 'SF3') if last in ('chain_stn', 'chain') else ('D1', 'D2', 'D3')
            r['tag'] = names[n] if n < 3 else None
            n += 1
            if r['tag'] == 'SF3' and last == 'chain':
                last = 'chain_stn'
    full = []
    for r in rows:
        t = r['tag']
        if t is None:
            continue
        # where the grid shows the chunk size: row tiles of 32, 64 or 128 queries, one thread per query in the tail
        if t in FC:
            r['full'] = (r['grid'][0] // r['wg']) in (CHUNK // 32, CHUNK // 64, CHUNK // 128)
        elif t == 'tail':
            r['full'] = r['grid'][0] == CHUNK
        full.append(r)
    return full


def summarise(rows):
    out = {}
    groups = {}
    for r in rows:
        groups.setdefault(r['tag'], []).append(r)
    # a launch of a ragged last chunk is left out by its duration for the kernels whose grid does not show the chunk size:
    # keep the launches within the upper half of the duration range of their layer where the grid says nothing
    for tag in ORDER:
        g = groups.get(tag)
        if not g:
            continue
        if tag in FC or tag == 'tail':
            g = [r for r in g if r['full']]
        else:
            top = statistics.median(r['end'] - r['start'] for r in g)
            g = [r for r in g if (r['end'] - r['start']) > 0.5 * top]
        if not g:
            continue
        d = [(r['end'] - r['start']) / 1e6 for r in g]
        gaps = [r['gap'] / 1e6 for r in g if 'gap' in r]
        nxt = statistics.mode(r['next'] for r in g if 'next' in r) if gaps else None
        e = {'launches': len(d), 'ms_median': round(statistics.median(d), 5), 'ms_mean': round(statistics.fmean(d), 5),
             'ms_stdev': round(statistics.pstdev(d), 5), 'ms_min': round(min(d), 5), 'ms_max': round(max(d), 5),
             'gap_to_next_ms_median': round(statistics.median(gaps), 5) if gaps else None, 'next_launch': nxt,
             'grid_threads': list(g[0]['grid']), 'workgroup': g[0]['wg'], 'vgpr': g[0]['vgpr'], 'agpr': g[0]['agpr'],
             'sgpr': g[0]['sgpr'], 'lds_bytes': g[0]['lds'], 'scratch': g[0]['scratch'], 'kernel': g[0]['name'][:80]}
        if tag in FC:
            n, k, z = FC[tag]
            flop = 2.0 * CHUNK * n * k * z
            e['gflop'] = round(flop / 1e9, 2)
            e['fraction_of_fp32_mfma_peak'] = round(flop / (e['ms_median'] * 1e-3) / PEAK, 3)
        out[tag] = e
    small = [t for t in out if not t.startswith('chain')]
    out['_small_kernels_ms_per_chunk'] = round(sum(out[t]['ms_median'] for t in small), 4)
    out['_small_kernel_gaps_ms_per_chunk'] = round(sum(out[t]['gap_to_next_ms_median'] or 0 for t in small), 4)
    out['_fc_ms_per_chunk'] = round(sum(out[t]['ms_median'] for t in FC if t in out), 4)
    return out


def main():
    rows = label(load(sys.argv[1]))
    out = summarise(rows)
    text = json.dumps(out, indent=1)
    if len(sys.argv) > 2:
        with open(sys.argv[2], 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
