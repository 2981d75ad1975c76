"""Which nodes of a chunk cross its boundary, from the chunk's own 257 adjacent deltas (csrc/lbvh.hip: the search workgroups of
k_chunk's launch find their nodes this way, the chunk workgroups by what the climb leaves unnamed).  Node t of the chunk at
c0 has dp = adj[t] = delta(c0 + t - 1, c0 + t) and dn = adj[t + 1]; it runs forward iff dn > dp, its threshold is the smaller
of the two, and it crosses iff every adjacent delta between it and the chunk's edge on that side -- adj[t + 1 .. 256] forward,
adj[0 .. t] backward -- exceeds the threshold (-1 where a neighbour does not exist).  Against the oracle's ranges, chunk by
chunk.  No GPU."""
import numpy as np
import pytest

from tests.test_cross_direct_unions import _codes
from tests.test_nodes_optional import _two_chains

C = 256
SIZES = [257, 513, 769, 256 * 11 + 1, 5000]
TWO_CHAINS_SIZES = SIZES + [700]           # (700: the size tests/test_lbvh_search_split.py builds on the GPU)
KINDS = ["uniform", "equal", "runs", "forty", "two_chains"]


def _clz32(x):
    x = np.asarray(x, np.uint64)
    out = np.full(x.shape, 32, np.int64)
    nz = x != 0
    out[nz] = 31 - np.floor(np.log2(x[nz].astype(np.float64))).astype(np.int64)      # exact below 2^53
    return out


def _adjacent(codes):
    """D[k] = delta(k - 1, k) for k = 0 .. n; -1 at both ends (collision.cl:65-77 with the position as the tie-break)."""
    n = len(codes)
    k = np.arange(1, n, dtype=np.uint64)
    a, b = codes[:-1].astype(np.uint64), codes[1:].astype(np.uint64)
    d = np.where(a != b, _clz32(a ^ b), 32 + _clz32((k - 1) ^ k))
    return np.concatenate([[-1], d, [-1]]).astype(np.int64)


def _criterion(D, n, chunk):
    c0 = chunk * C
    adj = np.full(C + 1, -1, np.int64)
    m = min(C + 1, n + 1 - c0)
    adj[:m] = D[c0:c0 + m]
    pre = np.minimum.accumulate(adj)                       # pre[t] = min adj[0 .. t]
    suf = np.minimum.accumulate(adj[::-1])[::-1]           # suf[t] = min adj[t .. 256]
    named = []
    for t in range(C):
        if c0 + t >= n - 1:
            break
        dp, dn = adj[t], adj[t + 1]
        thr = min(dp, dn)
        if (suf[t + 1] > thr) if dn > dp else (pre[t] > thr):
            named.append(c0 + t)
    return named


def _oracle_ranges(nodes, n):
    hi = nodes["right_edge"][:n - 1].astype(np.int64)
    cur = nodes["data"][:n - 1, 0].astype(np.int64)        # first leaf: follow the left children
    while (cur < n - 1).any():
        inner = cur < n - 1
        cur[inner] = nodes["data"][cur[inner], 0]
    return cur - (n - 1), hi


@pytest.mark.parametrize("kind,n", [(k, n) for k in KINDS for n in (TWO_CHAINS_SIZES if k == "two_chains" else SIZES)])
def test_adj_criterion_names_the_crossing_nodes(oracle, kind, n):
    assert 5000 % 256 == 136
    rs = np.random.RandomState(n % 100003 + len(kind))
    # (_two_chains lays out 358 codes before its filler: at 257 the first 257 of them, which are all equal)
    codes = _two_chains(max(n, 358))[:n] if kind == "two_chains" else _codes(kind, n, rs)
    ids = rs.permutation(n).astype(np.uint32)
    lo, hi = _oracle_ranges(oracle.build_bvh(codes, ids), n)
    crosses = (lo // C) != (hi // C)
    D = _adjacent(codes)
    total = 0
    for chunk in range((n + C - 1) // C):
        want = [i for i in range(chunk * C, min(chunk * C + C, n - 1)) if crosses[i]]
        assert _criterion(D, n, chunk) == want, "chunk %d" % chunk
        total += len(want)
    assert total == int(crosses.sum()) and total >= 1      # the root at least
