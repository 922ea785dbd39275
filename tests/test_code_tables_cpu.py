"""Character-code tables without a GPU: the table generators of tests/helpers.py build the shapes they claim, the oracle is a valid
referee for every shape (its lnL does not move when the codes are renumbered, and equals a numpy restatement of ConditionalPNode's tip
step on a small tree), and the engine's own numbering of the codes beyond 64 (code_order, paml_amd_debug_code_order) keeps the order
of a reference table exactly as it was and puts every state's single-state code at the state's position."""
import numpy as np
import pytest

import helpers
import oracle
from paml_amd import engine

SHAPES = helpers.CODE_TABLE_SHAPES
STATES = (4, 20, 61)


def _sets(n_chara, cmap):
    return [[int(x) for x in cmap[c, :n_chara[c]]] for c in range(len(n_chara))]


def _counts(n):
    return [c for c in (n, n + 3, 63, 64, 65, 128, 256) if c >= n]


def _cases():
    out = []
    for n in STATES:
        for s in SHAPES:
            for c in _counts(n):
                try:
                    helpers.code_table(n, c, s)
                except ValueError:
                    continue
                out.append((n, c, s))
    return out


CASES = _cases()


@pytest.mark.parametrize("n,n_codes,shape", CASES)
def test_code_table_has_the_shape_it_claims(n, n_codes, shape):
    n_chara, cmap, code_of = helpers.code_table(n, n_codes, shape, seed=n_codes)
    sets = _sets(n_chara, cmap)
    assert len(sets) == n_codes and all(len(set(s)) == len(s) for s in sets)      # (no state twice in a set)
    single = {}
    for c, s in enumerate(sets):
        if len(s) == 1:
            single.setdefault(s[0], []).append(c)
    plain = 0
    while plain < n and sets[plain] == [plain]:
        plain += 1
    amb = [s for s in sets if len(s) > 1]
    if shape == "reference":
        assert plain == n and all(s == sorted(s) for s in amb)
    if shape == "permuted":
        assert plain < n and sorted(sets[:n]) == [[s] for s in range(n)]
    if shape == "interleaved":
        assert len(sets[0]) == n and sorted(single) == list(range(n))
    if shape == "dup_single":
        assert plain == n and any(len(v) > 1 for v in single.values())
    if shape == "empty_unused":
        assert plain == n and any(len(s) == 0 for s in sets)
    if shape == "no_single":
        missing = sorted(set(range(n)) - set(single))
        assert len(missing) == 1 and any(missing[0] in s and len(s) < n for s in amb)
    if shape == "unordered":
        assert plain == n and amb and all(s != sorted(s) for s in amb)
    assert code_of == helpers.table_code_of(n_chara, cmap)
    assert all(sets[c] and frozenset(sets[c]) == k for k, cs in code_of.items() for c in cs)


@pytest.mark.parametrize("n,n_codes,shape", [c for c in CASES if c[1] in (c[0] + 3, 65)])
def test_with_code_table_keeps_every_cells_state_set(n, n_codes, shape):
    """Without the sprinkled ambiguity every cell keeps its state set, or (a state without a code of its own) takes the smallest set of
    the table that holds it; with it, every non-empty code occurs and no empty one."""
    pb = helpers.random_problem(n, 6, 80, seed=n, ambiguity=False)
    q = helpers.with_code_table(pb, n_codes, shape, seed=4, amb_rate=0.0)
    sets = _sets(q.n_chara, q.chara_map)
    smallest = {}
    for s in range(n):
        holds = [len(t) for t in sets if s in t]
        smallest[s] = min(holds)
    for (i, h), old in np.ndenumerate(pb.z):
        new = sets[q.z[i, h]]
        assert old in new and len(new) == smallest[old]
    r = helpers.with_code_table(pb, n_codes, shape, seed=4)
    assert set(np.unique(r.z)) == {c for c in range(n_codes) if q.n_chara[c] > 0}


def test_reference_tables():
    names, n_chara, cmap = helpers.nucleotide_table()
    assert len(names) == 18 and _sets(n_chara, cmap)[:6] == [[0], [1], [2], [3], [0], [0, 1]] and _sets(n_chara, cmap)[-3:] == [[0, 1, 2, 3]] * 3
    names, n_chara, cmap = helpers.amino_acid_table()
    assert len(names) == 24 and (n_chara[:20] == 1).all() and (n_chara[20:] == 20).all()
    names, n_chara, cmap = helpers.codon_amino_acid_table()
    sets = _sets(n_chara, cmap)
    assert len(sets) == 84 and sets[:61] == [[i] for i in range(61)] and sets[61:64] == [[], [], []]
    assert sorted(x for s in sets[64:] for x in s) == list(range(61)) and all(s == sorted(s) for s in sets[64:])
    assert [len(s) for s in sets[64:]] == [4, 6, 2, 2, 2, 2, 2, 4, 2, 3, 6, 2, 1, 2, 4, 6, 4, 1, 2, 4]      # (A R N D C Q E G H I L K M F P S T W Y V)


# ---- the oracle as referee --------------------------------------------------------------------------------------------------------------
def _numpy_lnl(pb):
    """ConditionalPNode (codeml.c:3535-3590) restated for one rate class: a tip son contributes, per pattern, the sum over its code's
    listed states of the P(t) column; the root's partials weighted by pi give f_h."""
    t, e = pb.tree, pb.eigen[0]
    U, V, R = e["U"], e["V"], e["Root"]

    def P(x):
        return (U * np.exp(R * t.branch[x])[None, :]) @ V

    def partial(x):
        L = np.ones((pb.n_patt, pb.n))
        for s in t.sons[x]:
            Ps = P(s)
            if not t.sons[s]:
                L *= np.stack([Ps[:, pb.chara_map[c, :pb.n_chara[c]]].sum(axis=1) for c in pb.z[s]])
            else:
                L *= partial(s) @ Ps.T
        return L
    f = partial(t.root) @ pb.pi[0]
    return float(np.dot(pb.weights, np.log(f))), np.log(f)


ORACLE_CASES = [c for c in CASES if c[1] in (c[0], c[0] + 3, 65, 256)]


@pytest.mark.parametrize("n,n_codes,shape", ORACLE_CASES)
def test_oracle_is_invariant_under_relabelling_and_matches_numpy(n, n_codes, shape):
    pb = helpers.with_code_table(helpers.random_problem(n, 6, 60, seed=3 + n), n_codes, shape, seed=n_codes)
    ref = oracle.evaluate(pb)
    rng = np.random.default_rng(n_codes)
    for _ in range(2):
        q = helpers.relabel_codes(pb, rng.permutation(n_codes))
        out = oracle.evaluate(q)
        assert out["lnL"] == ref["lnL"] and np.array_equal(out["lnf"], ref["lnf"])
    lnl, lnf = _numpy_lnl(pb)
    assert abs(lnl - ref["lnL"]) <= 1e-12 * abs(lnl) and np.max(np.abs(lnf - ref["lnf"])) < 1e-11


# ---- the engine's numbering of the codes beyond 64 ----------------------------------------------------------------------------------------
def _order_before(n, n_chara, cmap, z):
    """The numbering set_tips used before single-state codes were placed at their states (kept here as the yardstick for reference
    tables): the leading codes c = single state c stay, the others are sorted by (cells) x (set size), descending, stable."""
    n_codes = len(n_chara)
    plain = 0
    while plain < min(n, n_codes) and n_chara[plain] == 1 and cmap[plain, 0] == plain:
        plain += 1
    cnt = np.bincount(z.ravel(), minlength=n_codes)
    rest = sorted(range(plain, n_codes), key=lambda c: -int(cnt[c]) * int(n_chara[c]))      # (sorted() is stable)
    return list(range(plain)) + rest


@pytest.fixture(scope="module")
def lib_path():
    return engine.build()


@pytest.mark.parametrize("n,n_amb,seed", [(61, 10, 1), (61, 60, 2), (61, 190, 3), (33, 40, 4), (64, 9, 5)])
def test_code_order_of_a_reference_table_is_unchanged(lib_path, n, n_amb, seed):
    pb = helpers.random_problem(n, 12, 500, seed=seed, ambiguity=True, n_amb=n_amb, amb_rate=0.3)
    assert pb.n_codes > 64
    got = engine.debug_code_order(n, pb.n_chara, pb.chara_map, pb.z)
    assert got.tolist() == _order_before(n, pb.n_chara, pb.chara_map, pb.z)


@pytest.mark.parametrize("name", ["hiv_m3", "mhc_m0_scaled", "mtcdnapri_aadist1", "codon_amino_acid", "dup_single", "empty_unused"])
def test_code_order_of_the_reference_layouts_is_unchanged(lib_path, name):
    if name not in ("codon_amino_acid", "dup_single", "empty_unused"):      # the ambiguous codons of a golden alignment, numbered as the reference does
        z, n_chara, cmap = helpers.codon_codes_with_ambiguity(helpers.load_golden(name)["patterns_raw"])
        n = 61
        if len(n_chara) <= 64:      # (few ambiguous triplets: add codes the data do not use, as a larger alignment would have)
            n_chara = np.concatenate([n_chara, np.full(70 - len(n_chara), 61, dtype=np.int32)])
            cmap = np.concatenate([cmap, np.tile(np.arange(61, dtype=np.uint8), (70 - len(cmap), 1))])
    elif name == "codon_amino_acid":
        _, n_chara, cmap = helpers.codon_amino_acid_table()
        n = 61
        z = helpers.with_table(helpers.random_problem(61, 8, 300, seed=9), n_chara, cmap, seed=1).z
    else:
        n = 61
        q = helpers.with_code_table(helpers.random_problem(61, 8, 300, seed=9), 128, name, seed=2)
        n_chara, cmap, z = q.n_chara, q.chara_map, q.z
    got = engine.debug_code_order(n, n_chara, cmap, z)
    assert got.tolist() == _order_before(n, n_chara, cmap, z)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("n,n_codes", [(61, 65), (61, 128), (64, 256), (33, 70)])
def test_code_order_puts_every_single_state_code_at_its_state(lib_path, n, n_codes, shape):
    """Position s holds state s's first single-state code; the other codes follow by (cells) x (set size), descending, stable; a
    state without a code of its own gets one of those codes at its position (plain_codes < n: the per-tree kernel stays unused)."""
    pb = helpers.with_code_table(helpers.random_problem(n, 10, 400, seed=n_codes), n_codes, shape, seed=5)
    got = engine.debug_code_order(n, pb.n_chara, pb.chara_map, pb.z).tolist()
    assert sorted(got) == list(range(n_codes))
    first = {}
    for c in range(n_codes):
        if pb.n_chara[c] == 1:
            first.setdefault(int(pb.chara_map[c, 0]), c)
    cnt = np.bincount(pb.z.ravel(), minlength=n_codes)
    rest = sorted((c for c in range(n_codes) if c not in first.values()), key=lambda c: -int(cnt[c]) * int(pb.n_chara[c]))
    want, k = [], 0
    for pos in range(n_codes):
        if pos in first:
            want.append(first[pos])
        else:
            want.append(rest[k])
            k += 1
    assert got == want
    plain = 0
    while plain < n and pb.n_chara[got[plain]] == 1 and pb.chara_map[got[plain], 0] == plain:
        plain += 1
    assert (plain == n) == (shape != "no_single")
