"""The definition of read mapping (csrc/wn_readmap.hip) as plain loops over Python integers: minimizers of
a label row, the index of a reference, the anchors of a read, the chain table and the result of a read.  Nothing here is fast or
clever; tests/test_readmap_ref.py holds it to brute-force enumeration and to a case worked by hand, and the GPU tests hold the
kernels to it by exact equality, ties included.

Labels: 1..4 are bases whose complement is 5 - v; anything else is a break."""
INT_MIN = -2 ** 31
PAD = 2 ** 63 - 1
DEFAULTS = dict(k=15, w=10, max_occ=8, h=64, max_dist=5000, bandwidth=500, gap_base=2, gap_log=8, anchors_per_read=4096)


def fmix32(x):
    """murmur3's finaliser, a bijection on 32 bits"""
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def kmer(labels, p, k):
    """(canon, strand) of the k-mer at p, or None if it is invalid (a break in it, or a palindrome)"""
    f = r = 0
    for i in range(k):
        v = int(labels[p + i])
        if not 1 <= v <= 4:
            return None
        f += (v - 1) * 4 ** (k - 1 - i)
        r += (4 - v) * 4 ** i
    if f == r:
        return None
    return (min(f, r), 1 if r < f else 0)


def minimizers_ref(labels, k, w):
    """[(position, canon, strand)] in ascending position: p is a minimizer iff it holds a valid k-mer whose key (hash, p) is the
    lexicographic minimum over the valid k-mers of at least one window"""
    n = len(labels)
    n_k = n - k + 1
    if n_k < 1:
        return []
    codes = [kmer(labels, p, k) for p in range(n_k)]
    keys = [None if c is None else (fmix32(c[0]), p) for p, c in enumerate(codes)]
    out = []
    for p in range(n_k):
        if keys[p] is None:
            continue
        if n_k < w:
            starts, width = [0], n_k                         # the single window [0, n_k)
        else:
            starts = range(max(0, p - w + 1), min(p, n_k - w) + 1)
            width = w
        hit = False
        for s in starts:
            if all(keys[t] is None or keys[t] >= keys[p] for t in range(s, s + width)):
                hit = True
                break
        if hit:
            out.append((p, codes[p][0], codes[p][1]))
    return out


def index_ref(bases, k, w):
    """the reference's minimizers as (canon, pos, strand), sorted by (canon, pos)"""
    return sorted((c, p, s) for p, c, s in minimizers_ref(bases, k, w))


def anchors_ref(labels, index, k, w, max_occ, anchors_per_read):
    """(anchors [(s, r, q')] in enumeration order, cut to anchors_per_read; n_minimizers; truncated)"""
    n = len(labels)
    mins = minimizers_ref(labels, k, w)
    by_canon = {}
    for c, pos, s in index:                                  # sorted: ascending pos within a canon
        by_canon.setdefault(c, []).append((pos, s))
    out = []
    for q, c, s_read in mins:
        hits = by_canon.get(c, [])
        if len(hits) > max_occ:
            continue
        for pos, s_ref in hits:
            s = s_read ^ s_ref
            out.append((s, pos, q if s == 0 else n - k - q))
    truncated = 1 if len(out) > anchors_per_read else 0
    return out[:anchors_per_read], len(mins), truncated


def pack(anchor):
    s, r, q = anchor
    return (s << 43) | (r << 16) | q


def gap_cost(dd, gap_base, gap_log):
    return 0 if dd == 0 else gap_base * dd + gap_log * (dd.bit_length() - 1)


def chain_strand_ref(anchors, k, h, max_dist, bandwidth, gap_base, gap_log):
    """anchors [(r, q')] of ONE strand sorted by (r, q') -> (f, pred, root, count), pred -1 for a fresh start"""
    f, pred, root, count = [], [], [], []
    for i, (ri, qi) in enumerate(anchors):
        best = (16 * k, i)                                   # the fresh start is the candidate (16 k, i)
        for j in range(max(0, i - h), i):
            dr, dq = ri - anchors[j][0], qi - anchors[j][1]
            if not (0 < dr <= max_dist and 0 < dq <= max_dist):
                continue
            dd = abs(dr - dq)
            if dd > bandwidth:
                continue
            best = max(best, (f[j] + 16 * min(dr, dq, k) - gap_cost(dd, gap_base, gap_log), j))
        fresh = best[1] == i
        f.append(best[0])
        pred.append(-1 if fresh else best[1])
        root.append(i if fresh else root[best[1]])
        count.append(1 if fresh else count[best[1]] + 1)
    return f, pred, root, count


def chain_ref(sorted_anchors, n, k, h=64, max_dist=5000, bandwidth=500, gap_base=2, gap_log=8):
    """sorted_anchors: [(s, r, q')] sorted (forward strand first, each by (r, q')); n: the read's length.  Returns the result row as a
    dict, with f and pred over the whole sorted row (pred an index into that row, -1 for a fresh start)."""
    out = dict(score=INT_MIN, strand=-1, ref_start=-1, ref_end=-1, query_start=-1, query_end=-1, n_anchors=0, runner_up=INT_MIN, f=[], pred=[])
    if not sorted_anchors:
        return out
    nf = sum(1 for a in sorted_anchors if a[0] == 0)
    table = []                                               # (f, strand, i within the strand, root within the strand, count, r, q')
    for s, rows, off in ((0, sorted_anchors[:nf], 0), (1, sorted_anchors[nf:], nf)):
        part = [(r, q) for _, r, q in rows]
        f, pred, root, count = chain_strand_ref(part, k, h, max_dist, bandwidth, gap_base, gap_log)
        out["f"] += f
        out["pred"] += [-1 if p < 0 else p + off for p in pred]
        for i in range(len(part)):
            table.append((f[i], s, i, root[i], count[i], part))
    # the greatest f; ties to the forward strand, then to the smallest i
    best = max(table, key=lambda t: (t[0], -t[1], -t[2]))
    fb, s, i, root, count, part = best
    out.update(score=fb, strand=s, ref_start=part[root][0], ref_end=part[i][0] + k, n_anchors=count)
    if s == 0:
        out.update(query_start=part[root][1], query_end=part[i][1] + k)
    else:
        out.update(query_start=n - k - part[i][1], query_end=n - part[root][1])
    others = [t[0] for t in table if (t[1], t[3]) != (s, root)]
    out["runner_up"] = max(others) if others else INT_MIN
    return out


def map_read_ref(labels, index, max_len=None, **kw):
    """one read through all three steps at the given parameters (DEFAULTS for the rest); a length outside [0, max_len] is the caller's"""
    p = dict(DEFAULTS, **kw)
    anchors, n_min, truncated = anchors_ref(labels, index, p["k"], p["w"], p["max_occ"], p["anchors_per_read"])
    rows = sorted(anchors)
    out = chain_ref(rows, len(labels), p["k"], p["h"], p["max_dist"], p["bandwidth"], p["gap_base"], p["gap_log"])
    out.update(n_minimizers=n_min, truncated=truncated, keys=[pack(a) for a in rows], n_kept=len(rows))
    return out


def revcomp(seq):
    return [5 - int(v) if 1 <= int(v) <= 4 else int(v) for v in reversed(seq)]
