"""The looks of the resident head's polls PER WORKGROUP, paired by compute unit, at configs[1]: a -DLCF_POLL_LOOKS build of
the library (never shipped; see lcf_hip.hip) keeps, per workgroup and launch, the polls that were over after 1, 2, 3 and
more looks and where the workgroup ran (hardware-id register, XCC id).  Two workgroups of one launch at the same place
shared a compute unit for the whole launch; the one with the lower blockIdx.x was dispatched first and is the OLDER one.
Run with LCF_HIP_LIB=<that build> on the GPU box; writes one JSON file -- the summary over the pairs of every launch and
one row per compute unit, its launches summed -- and prints the summary.
    python tools/debug/poll_looks_by_cu.py [label] [out.json] [walkers=1024] [steps=1000]
`summarise(records)` is the arithmetic alone (tests/test_poll_looks_by_cu.py)."""
import json
import os
import sys

WORDS = 8   # launch, blockIdx.x, HW_ID, XCC_ID, polls of 1 / 2 / 3+ looks, looks in total


def place(hw_id, xcc_id):
    """(XCC, shader engine, shader array, compute unit) of gfx9's HW_ID: CU_ID bits 8-11, SH_ID bit 12, SE_ID bits 13-15."""
    return xcc_id & 15, (hw_id >> 13) & 7, (hw_id >> 12) & 1, (hw_id >> 8) & 15


def _wg(rec):
    one, two, more, looks = rec[4:8]
    polls = one + two + more
    return dict(block=rec[1], polls=polls, looks_1=one, looks=looks, looks_3_or_more=more,
                first_look_share=round(one / polls, 4) if polls else None,
                looks_per_poll=round(looks / polls, 4) if polls else None)


def _dist(v):
    v = sorted(v)
    if not v:
        return None
    q = lambda f: v[min(len(v) - 1, int(f * len(v)))]   # noqa: E731
    return dict(n=len(v), min=v[0], p10=q(0.1), p25=q(0.25), median=q(0.5), p75=q(0.75), p90=q(0.9), max=v[-1],
                mean=round(sum(v) / len(v), 4))


def summarise(records):
    """`records`: rows of WORDS integers.  -> (per-CU list, summary).  A CU of a launch is listed when exactly two of the
    launch's workgroups ran on it; the others are counted in the summary (`cus_not_paired`)."""
    cus = {}
    for r in records:
        cus.setdefault((r[0],) + place(r[2], r[3]), []).append(r)
    pairs, unpaired = [], 0
    for key in sorted(cus):
        wgs = sorted(cus[key], key=lambda r: r[1])
        if len(wgs) != 2 or not all(sum(w[4:7]) for w in wgs):
            unpaired += 1
            continue
        launch, xcc, se, sh, cu = key
        pairs.append(dict(launch=launch, xcc=xcc, se=se, sh=sh, cu=cu, older=_wg(wgs[0]), younger=_wg(wgs[1])))
    old = [p['older']['first_look_share'] for p in pairs]
    young = [p['younger']['first_look_share'] for p in pairs]
    d_old, d_young = _dist(old), _dist(young)
    summary = dict(workgroup_records=len(records), cu_pairs=len(pairs), cus_not_paired=unpaired,
                   first_look_share_older=d_old, first_look_share_younger=d_young)
    if pairs:
        # the spread within a group: its interquartile range; a CU's two workgroups "differ" when their shares are
        # further apart than the larger of the two spreads
        spread = max(d_old['p75'] - d_old['p25'], d_young['p75'] - d_young['p25'])
        diff = [y - o for o, y in zip(old, young)]
        more_old = sum(p['older']['looks_3_or_more'] for p in pairs)
        more_young = sum(p['younger']['looks_3_or_more'] for p in pairs)
        polls = sum(p['older']['polls'] + p['younger']['polls'] for p in pairs)
        summary.update(
            spread_within_group=round(spread, 4),
            share_of_cus_younger_above_older_by_more_than_spread=round(sum(d > spread for d in diff) / len(diff), 4),
            share_of_cus_older_above_younger_by_more_than_spread=round(sum(-d > spread for d in diff) / len(diff), 4),
            mean_younger_minus_older=round(sum(diff) / len(diff), 4),
            looks_per_poll_older=_dist([p['older']['looks_per_poll'] for p in pairs]),
            looks_per_poll_younger=_dist([p['younger']['looks_per_poll'] for p in pairs]),
            share_3_or_more=round((more_old + more_young) / polls, 4),
            share_of_the_3_or_more_on_older=round(more_old / max(1, more_old + more_young), 4))
    return pairs, summary


def by_cu(pairs):
    """The pairs of all launches, summed per compute unit: rows [xcc, se, sh, cu, launches, first-look share and looks per
    poll of the older workgroups, of the younger ones] -- a CU's older workgroup is another block in every launch."""
    acc = {}
    for p in pairs:
        a = acc.setdefault((p['xcc'], p['se'], p['sh'], p['cu']), [0] * 7)
        a[0] += 1
        for k, w in enumerate(('older', 'younger')):
            a[1 + 3 * k] += p[w]['polls']
            a[2 + 3 * k] += p[w]['looks_1']
            a[3 + 3 * k] += p[w]['looks']
    return [list(key) + [a[0], round(a[2] / a[1], 3), round(a[3] / a[1], 3), round(a[5] / a[4], 3), round(a[6] / a[4], 3)]
            for key, a in sorted(acc.items())]


def main():
    import ctypes as C
    sys.path.insert(0, os.getcwd())
    import bench
    from lightcurve_fitting_amd import engine as E
    label = sys.argv[1] if len(sys.argv) > 1 else 'build'
    path = sys.argv[2] if len(sys.argv) > 2 else 'poll_looks_by_cu.json'
    nw = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
    nst = int(sys.argv[4]) if len(sys.argv) > 4 else 1000
    model, lc, priors = bench.build_problem(0)
    eng = model.engine_for(lc, priors=priors)
    s = E.NativeSampler(eng, nw, 7)
    s.set_state(bench.initial_walkers(nw))
    s.run(0, 200, 'random', False)
    lib = E.load_library()
    cap = 16384
    out, n = (C.c_uint * (WORDS * cap))(), C.c_uint(0)
    lib.lcf_debug_read_poll_wg.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    assert lib.lcf_debug_read_poll_wg(out, cap, C.byref(n), 1) == 0
    s.run(200, nst, 'random', False)
    assert lib.lcf_debug_read_poll_wg(out, cap, C.byref(n), 0) == 0
    kept = min(n.value, cap)
    records = [[int(out[WORDS * k + j]) for j in range(WORDS)] for k in range(kept)]
    pairs, summary = summarise(records)
    x, lp = s.get_state()
    head = dict(build=label, walkers=nw, steps=nst, kernel=s.last_run_kernel(), launches=s.last_run_launches(),
                records_written=n.value, records_kept=kept, us_per_half_step=round(1e3 * s.last_run_ms() / (2 * nst), 3),
                mean_lp=round(float(lp.mean()), 6))
    head.update(summary)
    with open(path, 'w') as f:
        # (the summary is over the pairs of every launch; the rows are one per CU, its launches summed, as lists under
        # `columns`: the file stays small)
        columns = ['xcc', 'se', 'sh', 'cu', 'launches', 'older_first_look_share', 'older_looks_per_poll',
                   'younger_first_look_share', 'younger_looks_per_poll']
        json.dump(dict(summary=head, columns=columns, cus=by_cu(pairs)), f, separators=(',', ':'))
        f.write('\n')
    print(json.dumps(head))


if __name__ == '__main__':
    main()
