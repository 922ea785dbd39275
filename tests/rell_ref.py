"""numpy restatement of the bootstrap replicates of the tree comparison (paml_amd_rell_replicates): the counter-based generator, the
draw -> site -> pattern map and the replicate sums, from the description in paml_amd/csrc/kernels_rell.h and nothing else.

    mix(z)             = the SplitMix64 finaliser, arithmetic modulo 2^64
    stream(seed, r, g) = mix(seed + GAMMA * ((r << 32 | g) + 1))
    u(seed, r, g, j)   = mix(stream + GAMMA * (j + 1))
    site               = first site of gene g + ((u * lgene) >> 64)
The summation ORDER of the device is not restated: the sums here go through per-pattern counts, so results agree with the device's to
rounding (exactly, where every term is an integer)."""
import numpy as np

GAMMA = np.uint64(0x9E3779B97F4A7C15)
M1 = np.uint64(0xBF58476D1CE4E5B9)
M2 = np.uint64(0x94D049BB133111EB)
_LOW32 = np.uint64(0xFFFFFFFF)


def mix(z):
    z = np.atleast_1d(np.asarray(z, dtype=np.uint64)).copy()
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * M1
        z = (z ^ (z >> np.uint64(27))) * M2
    return z ^ (z >> np.uint64(31))


def stream(seed, r, g):
    with np.errstate(over="ignore"):
        packed = np.atleast_1d(np.uint64((int(r) << 32) | int(g))) + np.uint64(1)
        return mix(np.atleast_1d(np.uint64(int(seed) & (2 ** 64 - 1))) + GAMMA * packed)[0]


def mulhi(u, n):
    """High 64 bits of u * n for u uint64 and 0 < n < 2^32: neither partial product leaves 64 bits."""
    n = np.uint64(n)
    return ((u >> np.uint64(32)) * n + (((u & _LOW32) * n) >> np.uint64(32))) >> np.uint64(32)


def draws(seed, r, g, lgene):
    """Site index inside gene g (0 .. lgene - 1) of the draws j = 0 .. lgene - 1 of replicate r."""
    with np.errstate(over="ignore"):
        u = mix(np.atleast_1d(stream(seed, r, g)) + GAMMA * (np.arange(lgene, dtype=np.uint64) + np.uint64(1)))
    return mulhi(u, lgene).astype(np.int64)


def site_list(w):
    """site -> pattern: pattern h appears w[h] times, patterns of weight 0 never."""
    w = np.asarray(w).astype(np.int64)
    return np.repeat(np.arange(len(w), dtype=np.int64), w)


def gene_sites(w, gene_off=None):
    """First site of every gene (n_genes + 1 entries, the last = ls)."""
    w = np.asarray(w).astype(np.int64)
    go = [0, len(w)] if gene_off is None else list(gene_off)
    csum = np.concatenate([[0], np.cumsum(w)])
    return np.array([csum[o] for o in go], dtype=np.int64)


def replicate_patterns(w, gene_off, seed, r):
    """The ls patterns replicate r draws, genes one after the other."""
    sites, soff = site_list(w), gene_sites(w, gene_off)
    out = []
    for g in range(len(soff) - 1):
        lg = int(soff[g + 1] - soff[g])
        if lg:
            out.append(sites[soff[g] + draws(seed, r, g, lg)])
    return np.concatenate(out)


def counts(w, gene_off, seed, n_rep, first=0):
    """counts[r][h] = how often replicate first + r draws pattern h."""
    n_patt = len(w)
    return np.stack([np.bincount(replicate_patterns(w, gene_off, seed, first + r), minlength=n_patt) for r in range(n_rep)])


def replicates(lnf, w, gene_off=None, n_rep=1, seed=1, first=0):
    """(rep[n_rep][n_trees], mag[n_rep][n_trees]): the replicate sums and the sums of |lnf| over the same draws (the scale of the
    rounding error of any summation order)."""
    lnf = np.asarray(lnf, dtype=np.float64)
    c = counts(w, gene_off, seed, n_rep, first).astype(np.float64)
    return c @ lnf.T, c @ np.abs(lnf).T


def table_from_replicates(lnf, w, rep):
    """The columns of the comparison table from a replicate matrix rep[n_rep][n_trees], formula by formula (Kishino & Hasegawa 1989;
    Shimodaira & Hasegawa 1999; RELL with ties within 1e-5 shared)."""
    import math
    lnf, w, rep = np.asarray(lnf, dtype=np.float64), np.asarray(w, dtype=np.float64), np.asarray(rep, dtype=np.float64)
    n_trees, n_rep, ls = lnf.shape[0], rep.shape[0], w.sum()
    li = lnf @ w
    ml = int(np.argmax(li))      # the first of equal maxima
    dli = li - li[ml]
    y = lnf - lnf[ml]
    se = np.sqrt(((y - (dli / ls)[:, None]) ** 2) @ w)
    se[ml] = 0
    small = np.abs(se) < 1e-6
    pkh = np.array([-1.0 if (t == ml or small[t]) else 1 - 0.5 * math.erfc(dli[t] / se[t] / math.sqrt(2)) for t in range(n_trees)])
    prell = np.zeros(n_trees)
    for row in rep:
        yb, bt = row[0], [0]
        for t in range(1, n_trees):      # the reference's scan: a tree within 1e-5 of the running best joins it, a larger one replaces it
            if abs(row[t] - yb) < 1e-5:
                bt.append(t)
            elif row[t] > yb:
                yb, bt = row[t], [t]
        prell[bt] += 1.0 / (n_rep * len(bt))
    cen = rep - rep.mean(axis=0)
    mx = cen.max(axis=1)
    psh = np.array([np.count_nonzero(mx - cen[:, t] > li[ml] - li[t]) / n_rep for t in range(n_trees)])
    psh[ml] = -1
    psh[small] = -1
    return dict(li=li, dli=dli, se=se, pKH=pkh, pSH=psh, pRELL=prell, best=ml)
