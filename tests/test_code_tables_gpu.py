"""Character-code tables of every shape paml_amd_set_tips accepts (n_chara[code], chara_map[code][k]) on every kernel and entry point,
against the oracle.  The reference builds one layout — the single states first and in order, the ambiguous codes after them with their
states ascending (SetMapAmbiguity treesub.c:1218-1286) — and several fast paths lean on it: the P(t) kernel skips the map for the leading
single-state codes (plain_codes), the per-tree kernel adds up the rows of a code beyond the 64 of its ring block from the rows of the code's
states (jit_tip_overflow, device_common.h), and the branch-local and eigen-basis paths read a code's states as a bit mask.  Every case names
the kernel it must have run on, so that none passes by falling back to the interpreter.  Tables: tests/helpers.py (code_table, with_table,
relabel_codes)."""
import copy

import numpy as np
import pytest

import helpers
import oracle
from paml_amd import distributed
from paml_amd.engine import JIT, KEEP_PARTIALS, SHARD, EngineError, engine_for
from paml_amd.problem import Tree

pytestmark = pytest.mark.gpu

SHAPES = helpers.CODE_TABLE_SHAPES
MFMA_INTERP = {"mfma64_gather", "mfma64_stream"}
NOT_PER_TREE = MFMA_INTERP | {"mfma64_coop", "mfma64_coopjit"}      # (with the JIT flag small data sets then get the cooperative kernels)
INTERP = {4: {"valu4"}, 5: {"valu5"}, 20: {"valu20"}}
PER_TREE = {4: {"valu4_fused_jit", "valu4_jit"}, 5: {"valu5_fused_jit", "valu5_jit"}, 20: {"mfma4x20_jit", "valu20_jit"}}
# shapes that the 21..64-state per-tree kernel refuses beyond 64 codes: its overflow rows are the rows of the single states (a state
# without a code of its own has none) summed in ascending order (a set listed otherwise would give other bits than the interpreter's)
OVERFLOW_REFUSED = ("no_single", "unordered")


def base_problem(n, K=1, n_tips=12, n_patt=300, seed=None, **kw):
    return helpers.random_problem(n, n_tips, n_patt, K=K, seed=1000 + n if seed is None else seed, **kw)


def table_problem(n, n_codes, shape, K=1, seed=0, **kw):
    return helpers.with_code_table(base_problem(n, K=K, **kw), n_codes, shape, seed=seed)


def expected_kernels(n, n_codes, kind, shape="reference"):
    if kind == "interp":
        return INTERP.get(n, MFMA_INTERP)
    if kind in ("coop", "coopjit"):
        return {"mfma64_" + kind}
    if n in PER_TREE:
        return PER_TREE[n]
    return NOT_PER_TREE if (n_codes > 64 and shape in OVERFLOW_REFUSED) else {"mfma64_jit"}


def make_engine(pb, kind, monkeypatch, flags=0):
    """kind: interp (PAML_AMD_JIT=0 PAML_AMD_COOP=0), jit (the JIT flag), coop (the small-data interpreter, 21..64 states), coopjit (its
    per-tree form, compiled before the first evaluation)."""
    for v in ("PAML_AMD_JIT", "PAML_AMD_COOP", "PAML_AMD_JIT_SYNC"):
        monkeypatch.delenv(v, raising=False)
    if kind in ("interp", "coop"):
        monkeypatch.setenv("PAML_AMD_JIT", "0")
    if kind == "interp":
        monkeypatch.setenv("PAML_AMD_COOP", "0")
    if kind == "coopjit":
        monkeypatch.setenv("PAML_AMD_JIT_SYNC", "1")
    return engine_for(pb, flags=flags | (JIT if kind == "jit" else 0))


def check(pb, kind, monkeypatch, want, flags=0):
    """lnL to 1e-10 relative, every log f_h to 1e-9, fhK per class (as test_engine_gpu.check), and the kernel."""
    ref = oracle.evaluate(pb, want_fhk=True)
    eng = make_engine(pb, kind, monkeypatch, flags)
    out = eng.eval(pb.tree.branch, pb.gene_rate, want_lnf=True, want_fhk=True)
    assert eng.kernel_name in want, (eng.kernel_name, want)
    assert np.isfinite(out["lnL"])
    assert abs(out["lnL"] - ref["lnL"]) <= 1e-10 * abs(ref["lnL"]) + 1e-9, (out["lnL"], ref["lnL"], (out["lnL"] - ref["lnL"]) / abs(ref["lnL"]))
    assert np.max(np.abs(out["lnf"] - ref["lnf"])) < 1e-9, float(np.max(np.abs(out["lnf"] - ref["lnf"])))
    m = pb.weights > 0
    fk, rk = out["fhK"][:, m], ref["fhK"][:, m]
    tol = 1e-9 * np.abs(rk) + 1e-12 * np.abs(rk).max(axis=0, keepdims=True)
    assert (np.abs(fk - rk) <= tol).all(), float(np.max(np.abs(fk - rk) / np.abs(rk).max(axis=0, keepdims=True)))
    return eng, out, ref


# ---- state counts x kernels -----------------------------------------------------------------------------------------------------------
CODES_OF_N = {4: 18, 5: 8, 20: 24, 33: 70, 61: 84, 64: 128}      # (beyond 64 codes for every state count the 64-row ring block serves)
KERNEL_CASES = [(n, k) for n in CODES_OF_N for k in ("interp", "jit") + (("coop", "coopjit") if n > 20 else ())]


@pytest.mark.parametrize("n,kind", KERNEL_CASES)
def test_interleaved_table_on_every_kernel(n, kind, monkeypatch):
    """An interleaved table (code 0 = every state, the single states shuffled among the ambiguous codes) on the interpreter, the
    per-tree kernel and — 21..64 states — the small-data cooperative kernel and its per-tree form."""
    pb = table_problem(n, CODES_OF_N[n], "interleaved", K=2, seed=n)
    check(pb, kind, monkeypatch, expected_kernels(n, pb.n_codes, kind, "interleaved"))


# ---- shapes x code counts -------------------------------------------------------------------------------------------------------------
def _counts(n):
    return sorted({n, n + 3} | {c for c in (63, 64, 65, 128, 256) if c >= n})


def _valid(n, n_codes, shape):
    try:
        helpers.code_table(n, n_codes, shape)
        return True
    except ValueError:
        return False


# 61 states: every shape at every code count (the per-tree kernel's ring-block edge 64 / 65, the overflow path, the uint8 cap);
# 33 and 64 states and the 4 / 5 / 20-state kernels: every shape once and every code count once (33: n_codes 33 and 36 give an odd and
# an even TCH, jit.h — the tip-table chunks of the ring's DMA rounds)
SHAPE_CASES = [(61, c, s) for s in SHAPES for c in _counts(61) if _valid(61, c, s)]
for _n in (4, 5, 20, 33, 64):
    _cs = _counts(_n)
    SHAPE_CASES += [(_n, next(c for c in _cs[i % len(_cs):] + _cs if _valid(_n, c, s)), s) for i, s in enumerate(SHAPES)]
    SHAPE_CASES += [(_n, c, next(s for s in SHAPES[(j + 3) % len(SHAPES):] + SHAPES if _valid(_n, c, s))) for j, c in enumerate(_cs)]
SHAPE_CASES = sorted(set(SHAPE_CASES))


@pytest.mark.parametrize("n,n_codes,shape", SHAPE_CASES)
def test_table_shapes_and_code_counts_on_the_per_tree_kernel(n, n_codes, shape, monkeypatch):
    """Every table shape at n, n + 3, 63, 64, 65, 128 and 256 codes on the per-tree kernel of its state count; beyond 64 codes at 21..64
    states the tables without a single-state code for every state, or with a set out of ascending order, must get the interpreter."""
    pb = table_problem(n, n_codes, shape, seed=7 * n + n_codes)
    check(pb, "jit", monkeypatch, expected_kernels(n, n_codes, "jit", shape))


@pytest.mark.parametrize("shape", SHAPES)
def test_table_shapes_beyond_64_codes_on_the_interpreter(shape, monkeypatch):
    pb = table_problem(61, 128, shape, K=2, seed=3)
    check(pb, "interp", monkeypatch, MFMA_INTERP)


# ---- relabelling invariance -----------------------------------------------------------------------------------------------------------
RELABEL_CASES = [(4, 18, "interp"), (4, 18, "jit"), (5, 8, "jit"), (20, 24, "interp"), (20, 24, "jit"), (33, 36, "jit"), (33, 70, "jit"),
                 (61, 61, "jit"), (61, 84, "interp"), (61, 84, "jit"), (61, 128, "jit"), (61, 256, "jit"), (61, 84, "coop"), (61, 84, "coopjit"),
                 (64, 128, "jit")]


@pytest.mark.parametrize("n,n_codes,kind", RELABEL_CASES)
def test_relabelling_the_codes_gives_the_same_bits(n, n_codes, kind, monkeypatch):
    """Codes only index tip tables, and the engine's renumbering beyond 64 codes is meant to be invisible (set_tips): a permutation of
    the code numbers gives the same bits of lnL and of every log f_h on the same kernel.  (Beyond 64 codes which codes get ring-block rows
    depends on the numbering where counts tie; a row of the ring block and the overflow path's sum are the same additions in the same order
    — 0 + the rows of the states, ascending — so the bits do not move.)"""
    pb = table_problem(n, n_codes, "reference", K=2 if kind != "jit" else 1, seed=n_codes)
    rng = np.random.default_rng(n + n_codes)
    want = expected_kernels(n, n_codes, kind)
    ref = oracle.evaluate(pb)
    outs = []
    for perm in (np.arange(n_codes), rng.permutation(n_codes), rng.permutation(n_codes)):
        q = helpers.relabel_codes(pb, perm)
        assert oracle.evaluate(q)["lnL"] == ref["lnL"]
        eng = make_engine(q, kind, monkeypatch)
        out = eng.eval(q.tree.branch, q.gene_rate, want_lnf=True)
        assert eng.kernel_name in want, (eng.kernel_name, want)
        outs.append(out)
        eng.close()
    assert abs(outs[0]["lnL"] - ref["lnL"]) <= 1e-10 * abs(ref["lnL"])
    for o in outs[1:]:
        assert o["lnL"] == outs[0]["lnL"], (o["lnL"], outs[0]["lnL"])
        assert np.array_equal(o["lnf"], outs[0]["lnf"])


# ---- entry points with non-reference tables -------------------------------------------------------------------------------------------
ENTRY_TABLES = [("permuted", 0), ("interleaved", 3), ("permuted", 128), ("interleaved", 65)]      # (shape, n_codes; 0 / 3: n + 0 / n + 3)


def _codes(n, c):
    return n + c if c < 10 else c


def _with_branches(pb, br):
    q = copy.copy(pb)
    q.tree = Tree(pb.tree.n_tips, pb.tree.n_nodes, pb.tree.root, pb.tree.sons, np.asarray(br, dtype=np.float64).copy(), pb.tree.label)
    return q


@pytest.mark.parametrize("n", [4, 61])
@pytest.mark.parametrize("shape,c", ENTRY_TABLES)
def test_eval_branch_walk(n, shape, c, monkeypatch):
    """paml_amd_eval_branch at tip and internal branches, several trial lengths per call, against the oracle (lfuntdd)."""
    pb = table_problem(n, _codes(n, c), shape, K=2, n_tips=9, n_patt=150, seed=c)
    eng = make_engine(pb, "interp", monkeypatch)
    base = eng.eval(pb.tree.branch, pb.gene_rate)["lnL"]
    t = pb.tree
    for b in (0, 4, t.n_tips + 1, t.n_nodes - 1):
        if b == t.root:
            continue
        ts = np.array([t.branch[b], 0.02, 0.7])
        l, dl, ddl = eng.eval_branch(b, ts, t.branch, pb.gene_rate)
        rl, rdl, rddl = oracle.eval_branch(pb, b, ts)
        assert np.allclose(l, rl, rtol=1e-11, atol=0), (b, l, rl)
        assert np.allclose(dl, rdl, rtol=1e-9, atol=1e-9) and np.allclose(ddl, rddl, rtol=1e-9, atol=1e-8)
        assert abs(l[0] - base) <= 1e-11 * abs(base)
    assert eng.eval(pb.tree.branch, pb.gene_rate)["lnL"] == base


@pytest.mark.parametrize("shape,n_codes", [("permuted", 61), ("interleaved", 64), ("permuted", 128), ("interleaved", 65), ("no_single", 128)])
def test_eval_branch_refill_on_a_per_tree_kernel(shape, n_codes, monkeypatch):
    """The eval_branch refill (every length moved since the partials were formed) on its per-tree kernel, as in test_engine_gpu: l, l', l''
    against the oracle and the interpreter engine after two refills.  A table without a single-state code for every state keeps the refill
    on the interpreter beyond 64 codes (no refill kernel)."""
    pb = table_problem(61, n_codes, shape, K=1, n_patt=900, seed=5)
    t = pb.tree = copy.deepcopy(pb.tree)
    eng = make_engine(pb, "jit", monkeypatch)
    ref_eng = make_engine(pb, "interp", monkeypatch)
    fast = not (n_codes > 64 and shape in OVERFLOW_REFUSED)
    rng = np.random.default_rng(9)
    internal = [v for v in range(t.n_tips, t.n_nodes) if v != t.root]
    for rnd in range(2):
        t.branch[:] = np.where(np.arange(t.n_nodes) == t.root, 0.0, t.branch * rng.uniform(0.7, 1.4, t.n_nodes))
        for b in (internal[1], 2):
            ts = np.array([t.branch[b], 0.04, 0.6])
            l, dl, ddl = eng.eval_branch(b, ts, t.branch, pb.gene_rate)
            if b == internal[1]:
                assert eng.branch_counters()["refill_kernels"] == (rnd + 1 if fast else 0)
                if fast:
                    assert eng.kernel_name == "mfma64_jit", eng.kernel_name
            rl, rdl, rddl = oracle.eval_branch(pb, b, ts)
            il, idl, iddl = ref_eng.eval_branch(b, ts, t.branch, pb.gene_rate)
            assert np.allclose(l, rl, rtol=1e-11, atol=0), (rnd, b, l, rl)
            assert np.allclose(dl, rdl, rtol=1e-9, atol=1e-9) and np.allclose(ddl, rddl, rtol=1e-9, atol=1e-8)
            assert np.allclose(l, il, rtol=1e-12, atol=0) and np.allclose(dl, idl, rtol=1e-9, atol=1e-9)
    ref = oracle.evaluate(pb)["lnL"]
    assert abs(eng.eval(t.branch, pb.gene_rate)["lnL"] - ref) <= 1e-10 * abs(ref)


@pytest.mark.parametrize("n,kind", [(20, "interp"), (61, "interp"), (61, "jit")])
@pytest.mark.parametrize("shape,c", ENTRY_TABLES)
def test_keep_partials_and_dirty_eval(n, kind, shape, c, monkeypatch):
    """KEEP_PARTIALS: every internal node's partials against the oracle, then eval_dirty after one tip branch moved."""
    n_codes = _codes(n, c)
    pb = table_problem(n, n_codes, shape, K=2, n_tips=14, n_patt=150, seed=c, scale_every=4)
    ref = oracle.evaluate(pb, want_partials=True)
    want = expected_kernels(n, n_codes, kind, shape)
    eng, out, _ = check(pb, kind, monkeypatch, want, flags=KEEP_PARTIALS)
    t = pb.tree
    for node in range(t.n_tips, t.n_nodes):
        for ic in range(pb.K):
            assert np.allclose(eng.get_partials(node, ic), ref["partials"][ic, node - t.n_tips], rtol=1e-11, atol=1e-300)
    father = t.father()
    br = t.branch.copy()
    br[3] *= 1.7
    clean = np.ones(t.n_nodes, dtype=np.uint8)
    node = 3
    while node != -1:
        clean[node] = 0
        node = father[node]
    for _ in range(2):      # (a LOAD program gets its per-tree kernel from the second time it is asked for)
        got = eng.eval_dirty(br, clean)
        ref2 = oracle.evaluate(_with_branches(pb, br))["lnL"]
        assert abs(got - ref2) <= 1e-10 * abs(ref2), (got, ref2)


@pytest.mark.parametrize("n,kind", [(20, "jit"), (61, "interp"), (61, "jit")])
@pytest.mark.parametrize("shape,c", ENTRY_TABLES)
def test_eval_batch(n, kind, shape, c, monkeypatch):
    """paml_amd_eval_batch: every element (own branch lengths, class frequencies and rates) against the oracle."""
    n_codes = _codes(n, c)
    pb = table_problem(n, n_codes, shape, K=2, n_tips=10, n_patt=300, seed=c)
    eng, out, _ = check(pb, kind, monkeypatch, expected_kernels(n, n_codes, kind, shape))
    rng = np.random.default_rng(5)
    B = 4
    br = np.abs(pb.tree.branch[None, :] * (1 + 0.3 * rng.standard_normal((B, pb.tree.n_nodes))))
    br[0] = pb.tree.branch
    fk = rng.dirichlet(np.ones(pb.K), size=B)
    rt = pb.rate[None, :] * (1 + 0.2 * rng.random((B, pb.K)))
    fk[0], rt[0] = pb.freqK, pb.rate
    got = eng.eval_batch(br, gene_rate=np.tile(pb.gene_rate, (B, 1)), freqK=fk, rate=rt)
    assert got[0] == out["lnL"]
    for b in range(B):
        q = _with_branches(pb, br[b])
        q.freqK, q.rate = fk[b].copy(), rt[b].copy()
        r = oracle.evaluate(q)["lnL"]
        assert abs(got[b] - r) <= 1e-10 * abs(r), (b, got[b], r)


@pytest.mark.parametrize("shape,n_codes", [("permuted", 4), ("interleaved", 7), ("no_single", 18), ("unordered", 18)])
def test_eval_adg(shape, n_codes):
    """paml_amd_eval_adg (lfunAdG, 4 states) against the oracle."""
    from test_oracle_golden import _sites
    pb = table_problem(4, n_codes, shape, K=3, n_tips=9, n_patt=80, seed=21)
    rng = np.random.default_rng(4)
    pb.weights = rng.integers(1, 4, pb.n_patt).astype(float)
    pose = _sites(pb, rng)
    MK = 0.6 * np.eye(3) + 0.4 * rng.dirichlet(np.ones(3), size=3)
    eng = engine_for(pb)
    got = eng.eval_adg(pb.tree.branch, MK, pose, pb.gene_rate)
    ref = oracle.evaluate_adg(pb, MK, pose)
    assert abs(got - ref) <= 1e-10 * abs(ref), (got, ref)


@pytest.mark.parametrize("n", [4, 61])
@pytest.mark.parametrize("shape,c", ENTRY_TABLES)
def test_node_posterior(n, shape, c):
    """paml_amd_node_posterior at the root, a deep node and the last node against the oracle."""
    pb = table_problem(n, _codes(n, c), shape, K=2, n_tips=9, n_patt=140, seed=c)
    eng = engine_for(pb)
    base = eng.eval(pb.tree.branch, pb.gene_rate)["lnL"]
    for node in (pb.tree.root, pb.tree.n_tips + 1, pb.tree.n_nodes - 1):
        got = eng.node_posterior(node, pb.tree.branch, pb.gene_rate)
        ref = oracle.node_posterior(pb, node)
        assert np.allclose(got, ref, rtol=1e-9, atol=1e-13), (node, float(np.max(np.abs(got - ref))))
    assert eng.eval(pb.tree.branch, pb.gene_rate)["lnL"] == base


@pytest.mark.parametrize("shape,c", ENTRY_TABLES)
def test_beb_grid(shape, c, monkeypatch):
    """paml_amd_beb_grid on the class likelihoods of a non-reference table, against the numpy restatement of lfunNSsites_M2M8's sums
    (as test_engine_gpu.test_beb_grid_matches_numpy_restatement) over the ORACLE's class likelihoods."""
    K, ncls, ngrid = 7, 3, 300
    pb = table_problem(61, _codes(61, c), shape, K=K, n_tips=8, n_patt=1500, seed=31)
    rng = np.random.default_rng(8)
    pb.weights = rng.integers(0, 4, pb.n_patt).astype(float)
    eng, out, ref = check(pb, "interp", monkeypatch, MFMA_INTERP)
    pcl = rng.dirichlet(np.ones(ncls), size=ngrid)
    iw = rng.integers(0, K, size=(ngrid, ncls)).astype(np.int32)
    wc = np.linspace(0.1, 4.0, K)
    got = eng.beb_grid(pcl, iw, wc)
    m = pb.weights > 0
    f = ref["fhK"][:, m] / ref["fhK"][:, m].max(axis=0, keepdims=True)
    mix = np.einsum("gc,gch->gh", pcl, f[iw])
    lnfxs = (np.log(mix) * pb.weights[m]).sum(axis=1)
    fx = np.log(np.exp(lnfxs - lnfxs.max()).sum()) + lnfxs.max()
    t = pcl[:, :, None] * f[iw] / mix[:, None, :] * np.exp(lnfxs - fx)[:, None, None]
    m1 = (t * wc[iw][:, :, None]).sum(axis=(0, 1))
    assert abs(got["ln_fx"] - fx) <= 1e-9 * abs(fx)
    assert np.allclose(got["pr_last"][m], t[:, -1, :].sum(axis=0), rtol=1e-9, atol=1e-12)
    assert np.allclose(got["mean_w"][m], m1, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("n,kind", [(4, "jit"), (20, "jit"), (61, "interp"), (61, "jit")])
@pytest.mark.parametrize("shape,c", ENTRY_TABLES)
def test_several_genes(n, kind, shape, c, monkeypatch):
    """Three genes with their own models (Mgene 2-4) through a non-reference table."""
    n_codes = _codes(n, c)
    pb = table_problem(n, n_codes, shape, K=2, n_tips=10, n_patt=600, seed=c, n_genes=3)
    helpers.give_genes_their_own_models(pb, seed=n)
    check(pb, kind, monkeypatch, expected_kernels(n, n_codes, kind, shape))


@pytest.mark.parametrize("n", [4, 61])
@pytest.mark.parametrize("shape,c", ENTRY_TABLES)
def test_sharded_partial_sums_are_world_size_invariant(n, shape, c):
    """Pattern shards (SHARD) of a non-reference table: every shard engine renumbers its own codes by its own counts beyond 64 codes;
    the partial sums, added up, are the one-engine sums bit for bit for 2 and 3 shards."""
    pb = table_problem(n, _codes(n, c), shape, K=2, n_tips=10, n_patt=3000, seed=c)
    full = engine_for(pb)
    lnl = full.eval(pb.tree.branch, pb.gene_rate)["lnL"]
    assert abs(lnl - oracle.evaluate(pb, want_lnf=False)["lnL"]) <= 1e-10 * abs(lnl)
    pf = full.partial_sums()
    for world in (2, 3):
        tot = np.zeros_like(pf)
        for r in range(world):
            lo, hi = distributed.shard_bounds(pb.n_patt, world, r)
            sub = pb.slice_patterns(lo, hi)
            e = engine_for(sub, flags=SHARD)
            e.comm_init(0, 1, None, pb.n_patt, lo)
            e.eval(sub.tree.branch, sub.gene_rate)
            tot += e.partial_sums()
            e.close()
        assert np.array_equal(tot, pf)
        assert distributed.total_fixed_order(tot) == lnl


@pytest.mark.parametrize("n", [4, 20, 61])
@pytest.mark.parametrize("shape,c", ENTRY_TABLES + [("no_single", 3), ("no_single", 128), ("reference", 128)])
def test_get_pmat_on_a_tip_branch_is_right_or_refused(n, shape, c):
    """paml_amd_get_pmat of a tip branch rebuilds P from the tip's column table: it equals the oracle's P(t) to 1e-13 or is refused
    (EUNSUPPORTED) — never a wrong matrix.  Internal branches are always served."""
    pb = table_problem(n, _codes(n, c), shape, K=2, n_tips=8, n_patt=60, seed=c)
    eng = engine_for(pb)
    eng.eval(pb.tree.branch, pb.gene_rate)
    served = 0
    for node in (0, 3, pb.tree.n_tips + 1):
        for ic in range(pb.K):
            Pr = oracle.pmat_branch(pb, 0, ic, node)
            try:
                P = eng.get_pmat(0, ic, node)
            except EngineError as err:
                assert node < pb.tree.n_tips and "get_pmat" in str(err), str(err)
                continue
            assert np.max(np.abs(P - Pr)) < 1e-13, (node, ic, float(np.max(np.abs(P - Pr))))
            served += 1
    assert served >= pb.K
    if shape == "reference":
        assert served == 3 * pb.K


# ---- the reference's own tables -------------------------------------------------------------------------------------------------------
REF_TABLES = {"nucleotide": (4, helpers.nucleotide_table), "amino_acid": (20, helpers.amino_acid_table),
              "codon_amino_acid": (61, helpers.codon_amino_acid_table)}


@pytest.mark.parametrize("kind", ["interp", "jit"])
@pytest.mark.parametrize("name", list(REF_TABLES))
def test_reference_tables(name, kind, monkeypatch):
    """The reference's nucleotide (18 codes), amino-acid (24) and codon-based amino-acid (84: 61 .. 63 empty) tables, through the
    interpreter and the per-tree kernel, against the oracle."""
    n, table = REF_TABLES[name]
    _, n_chara, cmap = table()
    pb = helpers.with_table(base_problem(n, K=2), n_chara, cmap, seed=2)
    assert set(np.unique(pb.z)) == set(np.flatnonzero(n_chara))          # every non-empty code occurs, the empty ones never
    check(pb, kind, monkeypatch, expected_kernels(n, len(n_chara), kind))


# ---- a state listed twice in one set ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,n_codes", [(4, 7), (61, 64), (61, 70)])
def test_a_state_listed_twice_in_a_set_is_refused(n, n_codes):
    """The list-summing P(t) tables would count a repeated state twice (as ConditionalPNode does), the bit masks once: set_tips refuses
    such a set (PAML_AMD_EINVAL) and the engine stays usable."""
    pb = table_problem(n, n_codes, "reference", seed=1)
    bad_chara, bad_map = pb.n_chara.copy(), pb.chara_map.copy()
    c = n_codes - 1                                  # (an ambiguous set: its last state replaced by its first)
    assert bad_chara[c] >= 2
    bad_map[c, bad_chara[c] - 1] = bad_map[c, 0]
    eng = engine_for(pb)
    good = eng.eval(pb.tree.branch, pb.gene_rate)["lnL"]
    with pytest.raises(EngineError, match="twice"):
        eng.set_tips(pb.z, pb.weights, cleandata=0, n_chara=bad_chara, chara_map=bad_map)
    eng.set_tips(pb.z, pb.weights, cleandata=0, n_chara=pb.n_chara, chara_map=pb.chara_map)
    assert eng.eval(pb.tree.branch, pb.gene_rate)["lnL"] == good
