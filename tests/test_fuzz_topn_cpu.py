"""The generator of the structural fuzz of TopN / TopK / TopK-BSI on large fields (tests/fuzz_topn_gen.py) checked without a GPU: the
cases are deterministic in (seed, iteration); the default iterations reach every regime the GPU test exists for (walk_tags); the
candidate rule restated in numpy the way k_topn_candidates computes it (qualify, the cut (v, id_cut), T, later rows) equals the model
on every default case while each of eight wrong versions of it differs on at least one — so the inputs can tell a wrong kernel from a
right one; the pool bookkeeping gives oracle/pytopn.py's candidates on real column sets; and the TopK-BSI cases hold what they are for."""
import numpy as np
import pytest

import datagen as D
import fuzz_topn_gen as G
from oracle import pytopn as T

TAGS = {"stride2", "id_bin_hi", "id_bin_lo", "heap_exact", "heap_short", "heap_short_one_shard_only", "later_rows", "later_off_tanimoto", "ref_ne_exact",
        "cand_from_one_shard", "device_sort_default", "multi_pass", "tanimoto_nondegenerate"}
# wrong versions of the library's TopN, by the line they change (shard_candidates / library_topn below)
VARIANTS = ("id_low11",        # the index key of the tie selection cut to its low 11 bits
            "tie_desc",        # the tie at the cut broken by index descending
            "t_all",           # T over all qualifying rows instead of the first n
            "later_any_card",  # later rows admitted on their count alone, whatever their cardinality
            "later_tanimoto",  # later rows admitted under Tanimoto although T < min_threshold
            "n_a_256",         # the candidate kernel sees n_a rounded down to a multiple of 256
            "no_mask",         # the totals of non-candidates are not masked
            "order_desc")      # equal totals ordered by index descending


@pytest.fixture(scope="module")
def cases(oracle):
    return [G.Case(it) for it in range(6)]


def shard_candidates(cnt, count, src: int, has_src: bool, n: int, mt: int, tt: int, variant=None) -> np.ndarray:
    """k_topn_candidates for one shard: flags [n_a].  cnt, count: int64 [n_a]; mt as the caller passed it (0 stays 0)."""
    n_a = cnt.size
    idx = np.arange(n_a)
    tani = tt > 0 and has_src
    if tani:  # TopnRule::cnt_ok / count_ok
        cnt_ok = (cnt != 0) & ~((cnt * 100 <= src * tt) | (cnt * tt >= src * 100))
        den = np.maximum(cnt + src - count, 1)
        count_ok = (count != 0) & ((count * 100 + den - 1) // den > tt)
    else:
        cnt_ok, count_ok = (cnt != 0) & (cnt >= mt), (count != 0) & (count >= mt)
    seen = np.ones(n_a, dtype=bool)
    if variant == "n_a_256":
        seen[n_a // 256 * 256:] = False
    q = cnt_ok & count_ok & seen
    if int(q.sum()) < n:  # the heap never fills
        return q
    v = int(np.sort(cnt[q])[::-1][n - 1])  # the n-th qualifying row in rank order: its cardinality ...
    k = n - int((q & (cnt > v)).sum())
    tied = idx[q & (cnt == v)]
    if variant == "id_low11":
        id_cut = int(np.sort(tied & 2047)[k - 1])
    elif variant == "tie_desc":
        id_cut = int(tied[::-1][k - 1])
    else:
        id_cut = int(tied[k - 1])  # ... and, among the rows of that cardinality, its index
    first, past = (idx >= id_cut, idx < id_cut) if variant == "tie_desc" else (idx <= id_cut, idx > id_cut)
    in_p = q & ((cnt > v) | ((cnt == v) & first))
    pool_t = q if variant == "t_all" else in_p
    t = int(count[pool_t].min()) if pool_t.any() else 1 << 62
    later = has_src and (t >= mt or (variant == "later_tanimoto" and tani))
    flags = in_p.copy()
    if later:
        if variant == "later_any_card":
            flags |= ~in_p & (count >= t)
        elif variant == "later_no_cnt_ok":
            flags |= ~in_p & ((cnt < v) | ((cnt == v) & past)) & (count >= t)
        else:
            flags |= ~in_p & ((cnt < v) | ((cnt == v) & past)) & cnt_ok & (count >= t)
    return flags & seen


def library_topn(case, fld, si: int, variant=None):
    """fbk_topn under topn_semantics = 1 as the library computes it: per shard the counts of the rows that pass (k_topn_filter) and the
    candidate flags (k_topn_candidates), the totals masked (k_topn_mask) and ordered.  -> ((indexes, counts), flags [n_shards, n_a] or None)"""
    n, mt, tt, hf = fld.sets[si]
    ns, n_a = case.n_shards, fld.n_a
    cnt = fld.cnt.astype(np.int64)
    count = (fld.count_f if hf else fld.cnt).astype(np.int64)
    src = [int(x) for x in case.src_n] if hf else [0] * ns
    tot = np.zeros(n_a, dtype=np.int64)
    flags = np.zeros((ns, n_a), dtype=bool) if 0 < n < n_a else None
    for s in range(ns):
        if tt > 0 and hf:
            den = np.maximum(cnt[s] + src[s] - count[s], 1)
            ok = ~((cnt[s] * 100 <= src[s] * tt) | (cnt[s] * tt >= src[s] * 100)) & ((count[s] * 100 + den - 1) // den > tt)
        else:
            ok = (cnt[s] >= mt) & (count[s] >= mt)
        tot += np.where(ok & (cnt[s] != 0) & (count[s] != 0), count[s], 0)
        if flags is not None:
            flags[s] = shard_candidates(cnt[s], count[s], src[s], hf, n, mt, tt, variant)
    if flags is not None and variant != "no_mask":
        tot = np.where(flags.any(axis=0), tot, 0)
    idx = np.arange(n_a)
    order = np.lexsort((-idx if variant == "order_desc" else idx, -tot))
    order = order[tot[order] > 0][: n or None]
    return (order.tolist(), tot[order].tolist()), flags


def differs(case, fld, si: int, variant) -> bool:
    res, flags = library_topn(case, fld, si, variant)
    return res != fld.expect[(si, 1)] or (flags is not None and not np.array_equal(flags, fld.shard_cand[si]))


def test_cases_are_deterministic(cases, monkeypatch):
    a, b = cases[1], G.Case(1)
    assert np.array_equal(a.pool.words, b.pool.words) and np.array_equal(a.filter_words, b.filter_words) and np.array_equal(a.rf, b.rf)
    for fa, fb in zip(a.fields, b.fields):
        assert np.array_equal(fa.ra, fb.ra) and fa.sets == fb.sets and fa.expect == fb.expect
    x = G.BsiCase(65537)
    assert np.array_equal(x.ra, G.BsiCase(65537).ra)
    monkeypatch.setattr(D, "SEED", D.SEED + 1)
    c = G.Case(1)
    assert not np.array_equal(a.pool.words[:4], c.pool.words[:4]) and not np.array_equal(a.fields[0].ra, c.fields[0].ra)
    assert [f.n_a for f in c.fields] == [f.n_a for f in a.fields] and c.options == a.options and c.n_shards == a.n_shards, "the regime follows the iteration, not the seed"
    assert not np.array_equal(x.ra, G.BsiCase(65537).ra)


def test_default_iterations_cover_the_structure(cases):
    tags = [G.walk_tags(c) for c in cases]
    got = set().union(*tags)
    assert got >= TAGS, TAGS - got
    assert all("tanimoto_nondegenerate" in t for t in tags), "a Tanimoto set in which no shard has n qualifying rows"
    assert {f.n_a for c in cases for f in c.fields} == {255, 256, 257, 2047, 2049, 4096, 4097, 5003}
    assert {c.n_shards for c in cases} == {2, 3, 4}
    for c in cases:
        for f in c.fields:
            assert int(f.ra.max()) < len(c.pool.card) and f.ra.shape == (c.n_shards, f.n_a)
            assert 7 <= len(f.sets) <= 12 and all(0 < n < f.n_a for n, _, _, _ in f.sets), (c, f.sets)
            assert {tt for _, _, tt, _ in f.sets} - {0} <= {1, 20, 60}
        assert {tt for f in c.fields for _, _, tt, _ in f.sets} >= {1, 20, 60}, c
        res = [(f.sets[si][0], f.expect[(si, sem)][0]) for f in c.fields for si in range(len(f.sets)) for sem in (0, 1)]
        assert any(r for _, r in res) and any(len(r) < n for n, r in res), c  # some result non-empty, some shorter than n
        assert sorted(c.rf.tolist()) == list(range(c.n_shards))
        # the Tanimoto band of every shard holds at least a third of the pool, for every T
        for t in (1, 20, 60):
            for s in range(c.n_shards):
                src, card = int(c.src_n[s]), c.pool.card.astype(np.int64)
                assert 3 * int(((card * 100 > src * t) & (card * t < src * 100)).sum()) >= len(card), (c, t, s)
        # what the pool is made of: ties in cnt that carry different counts, cardinalities one apart and more than 2048 apart
        p = c.pool
        for g in p.group:
            assert len({int(p.card[r]) for r in g}) == 1 and all(len({int(pc[r]) for r in g}) >= 4 for pc in c.pool_count), c
        cut = p.group_card[G.CUT_GROUP]
        assert {cut - 1, cut + 1, cut + 2} <= {int(x) for x in p.card} and int(np.diff(np.unique(p.card)).max()) > 2048
        assert sum(r is not None for r in p.rows) == 40 and len(p.card) >= 190
    # at least 64 rows of group CUT in every field, on both sides of row 2048 where the field has both
    for c in cases:
        for f in c.fields:
            tied = (f.cnt == c.pool.group_card[G.CUT_GROUP]).sum(axis=1)
            assert f.cut_rows.size >= 64 and np.unique(f.cut_rows).size == f.cut_rows.size and (tied >= 64).all(), (c, f.n_a, f.cut_rows.size, tied)
            if f.n_a > 2048:
                assert (f.cut_rows < 2048).sum() >= 36 and (f.cut_rows >= 2048).sum() == min(36, f.n_a - 2048), (c, f.n_a)
    assert any((f.cut_rows >= 2048).sum() >= 36 for c in cases for f in c.fields)


@pytest.mark.parametrize("it", range(6))
def test_candidate_rule_in_numpy_equals_the_model(cases, it):
    c = cases[it]
    for f in c.fields:
        for si in range(len(f.sets)):
            res, flags = library_topn(c, f, si)
            assert f.from_shards(si, 1) == f.expect[(si, 1)] and f.from_shards(si, 0) == f.expect[(si, 0)], (c, f.n_a, si, f.sets[si])
            assert res == f.expect[(si, 1)], (c, f.n_a, si, f.why[si], f.sets[si])
            assert np.array_equal(flags, f.shard_cand[si]), (c, f.n_a, si, f.why[si], f.sets[si])


@pytest.mark.parametrize("variant", VARIANTS)
def test_every_wrong_version_is_caught_by_a_default_case(cases, variant):
    """later_any_card drops every test on the cardinality of a row outside the first n, the rank position included: the rule's own
    cnt_ok alone is implied by count >= T for the rows past the cut (T is the count of a row that passed count_ok, which puts it above
    src T% / 100 >= any count of a row below the band, and above min_threshold), so leaving only that out changes nothing."""
    caught = [(c.it, f.n_a, si) for c in cases for f in c.fields for si in range(len(f.sets)) if differs(c, f, si, variant)]
    assert caught, f"no default case tells the variant {variant} from the library"


def test_cnt_ok_of_a_later_row_is_implied_by_its_count(cases):
    """Why later_any_card is the variant above and not `the later rows without rule.cnt_ok(cnt)` alone: that one is the same function.
    A later row lies past the cut, so cnt <= v < the band's upper end; T is the count of a row p that passed count_ok, so
    T (100 + tt) > tt (cnt_p + src) > tt src (100 + tt) / 100, i.e. T > src tt / 100 >= the cardinality, hence the count, of any row at or
    below the band's lower end; without Tanimoto count >= T >= min_threshold gives cnt >= min_threshold.  Checked here on every case."""
    assert not [(c.it, f.n_a, si) for c in cases for f in c.fields for si in range(len(f.sets)) if differs(c, f, si, "later_no_cnt_ok")]


def test_candidates_equal_pytopn_on_column_sets(oracle):
    """one down-sized case (4096 columns, 255 rows) with the pool expanded to column sets: the per-shard candidates that the generator
    derives from (cardinality, count) pairs are oracle/pytopn.topn_candidates', and the results execute_topn's and top_exact's"""
    c = G.Case(0, sizes=(255,), universe=1 << 12, n_random=0)
    f = c.fields[0]
    cols = [set(np.nonzero(np.unpackbits(w.reshape(-1).view(np.uint8), bitorder="little"))[0].tolist()) for w in c.pool.words]
    fcols = [set(np.nonzero(np.unpackbits(c.filter_words[c.rf[s]].reshape(-1).view(np.uint8), bitorder="little"))[0].tolist()) for s in range(c.n_shards)]
    shards = [{r: cols[int(f.ra[s, r])] for r in range(f.n_a)} for s in range(c.n_shards)]
    assert [len(x) for x in fcols] == c.src_n.tolist()
    seen = 0
    for si, (n, mt, tt, hf) in enumerate(f.sets):
        srcs = fcols if hf else None
        assert np.nonzero(f.shard_cand[si].any(axis=0))[0].tolist() == T.topn_candidates(shards, n, srcs, mt, tt), (si, f.sets[si])
        for s in range(c.n_shards):
            one = T.topn_candidates(shards[s: s + 1], n, srcs[s: s + 1] if hf else None, mt, tt)
            assert np.nonzero(f.shard_cand[si][s])[0].tolist() == one, (si, s, f.sets[si])
            seen += len(one) > n
        assert list(zip(*f.expect[(si, 1)])) == T.execute_topn(shards, n, srcs, None, mt, tt), (si, f.sets[si])
        assert list(zip(*f.expect[(si, 0)])) == T.top_exact(shards, list(range(f.n_a)), n, srcs, mt, tt), (si, f.sets[si])
    assert seen, "no shard of the down-sized case returns later rows"


@pytest.mark.parametrize("n_a", G.BSI_SIZES)
def test_bsi_cases(oracle, n_a):
    c = G.BsiCase(n_a)
    assert c.ra.shape == (c.n_shards, n_a) and int(c.ra.max()) < len(c.pool.card) and c.n_shards in (2, 3)
    w = c.pool.words.reshape(len(c.pool.card), -1)
    tot = np.zeros(n_a, dtype=np.uint64)
    for s in range(c.n_shards):  # the totals from the words, 4096 rows at a time
        fw = c.filter_words[c.rf[s]].reshape(-1)
        pc = np.bitwise_count(w & fw).sum(axis=1).astype(np.uint64)
        tot += pc[c.ra[s]]
    assert np.array_equal(tot, c.tot)
    dec = G.decode_planes(c.planes)
    assert np.array_equal(dec[:n_a], c.tot) and not dec[n_a:].any()
    assert c.planes.shape[0] == int(c.tot.max()).bit_length() and c.planes[-1].any()
    x, y = c.split
    assert x and y and sorted(x + y) == list(range(c.n_shards))
    dx, dy = (int(c.shard_tot[z].sum(axis=0).max()).bit_length() for z in (x, y))
    assert dx != dy and min(dx, dy) > 0, (dx, dy)
    assert c.tot[n_a - 1] != 0, "no bit in the last word of the planes"
    if n_a > 65536:
        assert c.tot[65536:].any(), "no bit in slot 1 or higher"
    if n_a % 64:
        assert c.planes.reshape(c.planes.shape[0], -1)[:, n_a // 64].any(), "nothing in the last partial word"
    assert np.array_equal(c.tot[c.order[:-1]] >= c.tot[c.order[1:]], np.ones(c.order.size - 1, dtype=bool))
    assert np.unique(c.tot[c.order[:200]]).size < 200, "no equal totals at the top of the order"
    if n_a == 131077:
        assert np.unique(c.tot[c.order[:10]]).size < 10, "no equal totals among the first ten of the order"
        assert np.unique(G.top_of(c.pool.card[c.ra].sum(axis=0), 10)[1]).size < 10, "no equal cardinality totals among the first ten"


def test_bsi_sizes_cross_the_edges():
    assert G.BSI_SIZES == (65536, 65537, 131077, 1 << 20)
    assert any(n % 64 for n in G.BSI_SIZES) and any(n > 65536 and n % 65536 for n in G.BSI_SIZES)
