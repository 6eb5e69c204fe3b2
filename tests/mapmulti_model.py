"""A plain-Python restatement of the mapper's rule for more chains per read (include/np2_io.h, "More chains"), on top of
map_model's anchors and chaining recurrence and independent of the C++: the primary chain as map_model.map_read finds it, the
further selections over the unmarked anchors, the classes against the earlier parents on forward read coordinates, s2 and
mapq per class, the units and the PAF lines."""
import numpy as np

import map_model as mm

MULTI_DEFAULTS = dict(max_chains=1, supplementary=0, secondary_n=0, mask_pm=500, pri_pm=800)
PRIMARY, SUPPLEMENTARY, SECONDARY = 0, 1, 2
COUNTS = ("selections", "dropped_min_cnt", "dropped_secondary", "kept_supplementary", "kept_secondary")


def multi(**kw):
    m = dict(MULTI_DEFAULTS)
    m.update(kw)
    return m


def _sweep(p, f, marked):
    """base[] over the unmarked anchors against the marks"""
    base = np.zeros(len(p), np.int64)
    for i in np.flatnonzero(~marked):
        if p[i] < 0:
            base[i] = 0
        elif marked[p[i]]:
            base[i] = f[p[i]]
        else:
            base[i] = base[p[i]]
    return base


def _hit(path, rel, tid, r, q, qlen, k, s1):
    first, last = path[0], path[-1]
    q0, q1 = int(q[first]) - k + 1, int(q[last]) + 1
    ts, te = int(r[first]) - k + 1, int(r[last]) + 1
    rev = int(rel[first])
    qs, qe = (qlen - q1, qlen - q0) if rev else (q0, q1)
    matches = k
    for a, b in zip(path[:-1], path[1:]):
        matches += int(min(k, r[b] - r[a], q[b] - q[a]))
    return dict(tid=int(tid[first]), qlen=qlen, qs=qs, qe=qe, rev=rev, ts=ts, te=te, matches=matches, block=max(qe - qs, te - ts), mapq=0,
                n=len(path), s1=int(s1), s2=0)


def mapq_of(s1, s2, n):
    return min(60, (60 * max(s1 - s2, 0) // s1) * min(n, 10) // 10) if s1 else 0


def map_read(index, read, o, m, info=None):
    """-> (units, counts): units is a list of dicts with hit (None for an unmapped primary), cls, parent, chain ([n, 2] int64),
    the primary first.  info (a dict): "anchors" the read's anchor count, "non_monotone" anchors with f[i] < f[p[i]],
    "scores" the further selections' scores in order"""
    k = o["k"]
    cnt = dict.fromkeys(COUNTS, 0)
    rel, tid, r, q, _, _ = mm.anchors(index, read, o)
    if info is not None:
        info["anchors"] = len(r)
    unmapped = [dict(hit=None, cls=PRIMARY, parent=0, chain=np.zeros((0, 2), np.int64))]
    if len(r) == 0:
        return unmapped, cnt
    f, p = mm.chain(rel, tid, r, q, o)
    # the primary chain, as the chain rule has it (test_mapmulti_cpu.py holds it against map_model.map_read)
    marked = np.zeros(len(r), bool)
    path = []
    i = int(f.argmax())
    s1 = int(f[i])
    while i >= 0:
        marked[i] = True
        path.append(i)
        i = int(p[i])
    path = path[::-1]
    if len(path) < o["min_cnt"] or s1 < o["min_score"]:
        return unmapped, cnt
    qlen = len(read)
    hit0 = _hit(path, rel, tid, r, q, qlen, k, s1)
    free = np.flatnonzero(~marked)
    hit0["s2"] = max(0, int((f - _sweep(p, f, marked))[free].max())) if len(free) else 0
    hit0["mapq"] = mapq_of(s1, hit0["s2"], len(path))
    units = [dict(hit=hit0, cls=PRIMARY, parent=0, chain=np.stack([r[path], q[path]], axis=1))]
    if info is not None:
        has = p >= 0
        info["non_monotone"] = int(np.count_nonzero(f[has] < f[p[has]]))
        info["scores"] = []
    # parents: [qs, qe, s1, s2, kept secondaries, unit or None]
    parents = [[hit0["qs"], hit0["qe"], hit0["s1"], hit0["s2"], 0, 0]]
    for _ in range(m["max_chains"] - 1):
        free = np.flatnonzero(~marked)
        if len(free) == 0:
            break
        base = _sweep(p, f, marked)
        score = (f - base)[free]
        end = int(free[int(score.argmax())])  # the first maximum: the smallest i
        s1 = int(score.max())
        if s1 < o["min_score"]:
            break
        if info is not None:
            info["scores"].append(s1)
        cnt["selections"] += 1
        path = []
        i = end
        while i >= 0 and not marked[i]:
            marked[i] = True
            path.append(i)
            i = int(p[i])
        path = path[::-1]
        if len(path) < o["min_cnt"]:
            cnt["dropped_min_cnt"] += 1
            continue
        h = _hit(path, rel, tid, r, q, qlen, k, s1)
        chain = np.stack([r[path], q[path]], axis=1)
        for P in parents:
            ov = max(0, min(h["qe"], P[1]) - max(h["qs"], P[0]))
            if ov * 1000 > m["mask_pm"] * min(h["qe"] - h["qs"], P[1] - P[0]):
                if P is not parents[0]:
                    P[3] = max(P[3], s1)
                if P[5] is not None and s1 * 1000 >= m["pri_pm"] * P[2] and P[4] < m["secondary_n"]:
                    P[4] += 1
                    cnt["kept_secondary"] += 1
                    units.append(dict(hit=h, cls=SECONDARY, parent=P[5], chain=chain))
                else:
                    cnt["dropped_secondary"] += 1
                break
        else:
            me = [h["qs"], h["qe"], s1, 0, 0, None]
            parents.append(me)
            if m["supplementary"]:
                me[5] = len(units)
                cnt["kept_supplementary"] += 1
                units.append(dict(hit=h, cls=SUPPLEMENTARY, parent=len(units), chain=chain))
    for P in parents[1:]:
        if P[5] is not None:
            h = units[P[5]]["hit"]
            h["s2"] = P[3]
            h["mapq"] = mapq_of(h["s1"], h["s2"], h["n"])
    return units, cnt


def map_reads(index, reads, m, info=None, **kw):
    """-> (units per read: a list of lists, counts summed); info: a list that takes one dict per read"""
    o = mm.opts(k=index.k, w=index.w, **kw)
    out, tot = [], dict.fromkeys(COUNTS, 0)
    for rd in reads:
        one = {} if info is not None else None
        units, cnt = map_read(index, rd, o, m, one)
        if info is not None:
            info.append(one)
        out.append(units)
        for key, v in cnt.items():
            tot[key] += v
    return out, tot


def paf_line(qname, unit, tname, tlen):
    line = mm.paf_line(qname, unit["hit"], tname, tlen)
    return line.replace("\ttp:A:P\t", "\ttp:A:S\t") if unit["cls"] == SECONDARY else line


def paf(names, units, tnames, tlens):
    return "".join(paf_line(nm, u, tnames[u["hit"]["tid"]], tlens[u["hit"]["tid"]]) for nm, us in zip(names, units) for u in us if u["hit"])


def check(got, units, reads):
    """an implementation's (unit_off, hits, cls, parent[, chain, chain_off]) against the model's units"""
    unit_off, hits, cls, parent = got[:4]
    want_off = np.concatenate(([0], np.cumsum([len(us) for us in units]))).astype(np.uint64)
    assert np.array_equal(unit_off, want_off), (unit_off, want_off)
    flat = [(i, u) for i, us in enumerate(units) for u in us]
    assert len(hits) == len(flat) == len(cls) == len(parent)
    for t, (i, u) in enumerate(flat):
        g = hits[t]
        assert int(g["qlen"]) == len(reads[i]), (i, t)
        if u["hit"] is None:
            assert int(g["tid"]) == -1, (i, t, g)
        else:
            assert {f: int(g[f]) for f in mm.HIT_FIELDS} == u["hit"], (i, t, g, u["hit"])
        assert (int(cls[t]), int(parent[t])) == (u["cls"], u["parent"]), (i, t)
    if len(got) > 4:
        chain, chain_off = got[4], got[5]
        want = np.concatenate(([0], np.cumsum([len(u["chain"]) for _, u in flat]))).astype(np.uint64)
        assert np.array_equal(chain_off, want)
        rows = np.concatenate([u["chain"] for _, u in flat]) if flat else np.zeros((0, 2), np.int64)
        assert np.array_equal(chain.astype(np.int64), rows.reshape(-1, 2))


# ---- the units aligned, and their SAM (np2_io.h, "More chains": Alignment, SAM) ---------------------------------------------------
def align_units(contigs, reads, units, k, **akw):
    """every unit aligned with align_model.align_read (its own hit, its own chain) and the read's units settled: a read whose
    primary is unmapped or overflows keeps its primary alone, a further unit that overflows is dropped, and so is a secondary
    whose parent was.  -> (units per read with rec, cigar, md, cs, split added and parents renumbered, further units dropped)"""
    import align_model as am
    import aligntags_model as tm
    o = am.opts(**akw)
    cc = [am.codes(c) for c in contigs]
    cnt = dict.fromkeys(am.COUNT_FIELDS, 0)
    out, dropped = [], 0
    for rd, us in zip(reads, units):
        kept, place = [], {}
        for t, u in enumerate(us):
            rec = cg = None
            if u["hit"] is not None:
                rec, cg = am.align_read(cc[u["hit"]["tid"]], rd, u["hit"], u["chain"], k, o, cnt)
            ok = t == 0 or (0 in place and rec is not None and (u["cls"] != SECONDARY or u["parent"] in place))
            if t == 0 and rec is None:
                kept.append(dict(u, rec=dict(am.UNALIGNED), cigar=[], md=b"", cs=b"", split=[], parent=0))
                continue
            if not ok:
                dropped += 1
                continue
            place[t] = len(kept)
            seq = mm.revcomp(rd) if rec["flag"] & 16 else bytes(rd)
            md, cs, split = tm.tags(contigs[rec["tid"]][rec["pos"]:], seq, cg)
            parent = 0 if t == 0 else place[u["parent"]] if u["cls"] == SECONDARY else len(kept)
            kept.append(dict(u, rec=rec, cigar=cg, md=md, cs=cs, split=split, parent=parent))
        out.append(kept)
    return out, dropped


def _cigar_text(cg):
    return "".join(f"{n}{op}" for op, n in cg)


def sam_lines(qname, read, qual, us, tnames, md=False, cs=False, eqx=False):
    """one read's SAM lines from its aligned units: FLAG | 2048 / 256, full SEQ and QUAL, and SA:Z: last when the read has two
    or more aligned parent-class records"""
    read = bytes(read)
    if us[0]["rec"]["tid"] < 0:
        return [f"{qname}\t4\t*\t0\t0\t*\t*\t0\t0\t{read.decode() or '*'}\t{qual.decode() if qual else '*'}\n"]
    par = [u for u in us if u["cls"] != SECONDARY]
    lines = []
    for u in us:
        rec, hit = u["rec"], u["hit"]
        rev = bool(rec["flag"] & 16)
        seq = mm.revcomp(read) if rev else read
        ql = "*" if not qual else (qual[::-1] if rev else qual).decode()
        flag = rec["flag"] | (2048 if u["cls"] == SUPPLEMENTARY else 256 if u["cls"] == SECONDARY else 0)
        f = [qname, flag, tnames[rec["tid"]], rec["pos"] + 1, rec["mapq"], _cigar_text(u["split"] if eqx else u["cigar"]), "*", 0, 0, seq.decode(), ql,
             f"NM:i:{rec['nm']}", f"AS:i:{rec['as']}", f"cm:i:{hit['n']}", f"s1:i:{hit['s1']}", f"s2:i:{hit['s2']}"]
        if md:
            f.append("MD:Z:" + u["md"].decode())
        if cs:
            f.append("cs:Z:" + u["cs"].decode())
        if len(par) >= 2 and u["cls"] != SECONDARY:
            f.append("SA:Z:" + "".join(f"{tnames[v['rec']['tid']]},{v['rec']['pos'] + 1},{'-' if v['rec']['flag'] & 16 else '+'},"
                                       f"{_cigar_text(v['cigar'])},{v['rec']['mapq']},{v['rec']['nm']};" for v in par if v is not u))
        lines.append("\t".join(str(x) for x in f) + "\n")
    return lines


def sam(names, reads, quals, aligned, tnames, tlens, **flags):
    import align_model as am
    quals = quals or [None] * len(reads)
    return am.sam_header(tnames, tlens) + "".join("".join(sam_lines(n, r, q, us, tnames, **flags)) for n, r, q, us in zip(names, reads, quals, aligned))


def check_aligned(got, aligned, md=False, cs=False, eqx=False):
    """an aligned _m door's dict against the model's aligned units"""
    import align_model as am
    flat = [u for us in aligned for u in us]
    assert np.array_equal(got["unit_off"], np.concatenate(([0], np.cumsum([len(us) for us in aligned]))).astype(np.uint64))
    assert len(got["recs"]) == len(flat)
    for t, u in enumerate(flat):
        assert (int(got["cls"][t]), int(got["parent"][t])) == (u["cls"], u["parent"]), t
        if u["hit"] is not None:
            assert {f: int(got["hits"][t][f]) for f in mm.HIT_FIELDS} == u["hit"], t
        cg = u["split"] if eqx else u["cigar"]
        want = dict(u["rec"], n_cigar=len(cg))
        assert {f: int(got["recs"][t][f]) for f in am.REC_FIELDS} == {f: want[f] for f in am.REC_FIELDS}, (t, got["recs"][t], want)
        w = got["cigar"][int(got["cigar_off"][t]):int(got["cigar_off"][t + 1])]
        assert [("MIDNSHP=X"[int(x) & 15], int(x) >> 4) for x in w] == [tuple(c) for c in cg], t
        if md:
            assert got["md"][t] == u["md"], t
        if cs:
            assert got["cs"][t] == u["cs"], t
