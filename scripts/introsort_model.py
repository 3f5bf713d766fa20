"""The order libstdc++'s std::sort leaves on (key, index) pairs compared by key only, restated from the shape of its
introsort (median-of-3 to first, unguarded Hoare partition, heap sort at the depth limit 2*floor(log2 n), final
insertion sort with a threshold of 16) in the closed form the GPU kernels use (fastdem_amd/csrc/fdm_introsort.hpp).

One partition step on [f, l) with pivot p = key[f] after the median moved there: positions of [f+1, l) with key >= p
from the left (g_1 < g_2 < ...) pair with positions of key <= p from the right (r_1 > r_2 > ...); pair k swaps iff
g_k < r_k (K swaps, a prefix), and the cut is min(g_{K+1}, r_K), or g_1 if K = 0.  Ranges of <= 16 elements end
stably sorted (the insertion pass never crosses a partition boundary).

    python scripts/introsort_model.py      # checks the model against a literal run and the oracle's std::sort
"""
import sys

THRESHOLD = 16


def median_to_first(k, a, b, c):
    """__move_median_to_first(first, a, b, c) on keys k: the position whose element is swapped into first."""
    if k[a] < k[b]:
        if k[b] < k[c]:
            return b
        return c if k[a] < k[c] else a
    if k[a] < k[c]:
        return a
    return c if k[b] < k[c] else b


def partition_closed(k, f, l):
    """Cut of the unguarded partition of [f+1, l) around k[f], and the swapped pairs, in closed form."""
    p = k[f]
    g = [i for i in range(f + 1, l) if not (k[i] < p)]
    r = [i for i in range(l - 1, f, -1) if not (p < k[i])]
    K = 0
    while K < min(len(g), len(r)) and g[K] < r[K]:
        K += 1
    if K == 0:
        cut = g[0]
    else:
        cut = min(g[K], r[K - 1]) if K < len(g) else r[K - 1]
    return cut, list(zip(g[:K], r[:K]))


def partition_literal(k, f, l):
    """__unguarded_partition(f+1, l, f) as the loop it is (checks partition_closed)."""
    k = list(k)
    p = k[f]
    first, last, swaps = f + 1, l, []
    while True:
        while k[first] < p:
            first += 1
        last -= 1
        while p < k[last]:
            last -= 1
        if not first < last:
            return first, swaps
        k[first], k[last] = k[last], k[first]
        swaps.append((first, last))
        first += 1


def adjust_heap(a, base, hole, n, value):
    """__adjust_heap (and the __push_heap it ends with) on a[base : base + n], a list of (key, index) pairs."""
    top = hole
    child = hole
    while child < (n - 1) // 2:
        child = 2 * (child + 1)
        if a[base + child][0] < a[base + child - 1][0]:
            child -= 1
        a[base + hole] = a[base + child]
        hole = child
    if (n & 1) == 0 and child == (n - 2) // 2:
        child = 2 * (child + 1)
        a[base + hole] = a[base + child - 1]
        hole = child - 1
    parent = (hole - 1) // 2
    while hole > top and a[base + parent][0] < value[0]:
        a[base + hole] = a[base + parent]
        hole = parent
        parent = (hole - 1) // 2
    a[base + hole] = value


def heap_sort(a, f, l):
    """__partial_sort(f, l, l): __make_heap, then __sort_heap."""
    n = l - f
    if n < 2:
        return
    parent = (n - 2) // 2
    while True:
        adjust_heap(a, f, parent, n, a[f + parent])
        if parent == 0:
            break
        parent -= 1
    while n > 1:
        n -= 1
        value = a[f + n]
        a[f + n] = a[f]
        adjust_heap(a, f, 0, n, value)


def std_sort(keys, report=None):
    """Indices 0..n-1 in the order std::sort leaves the pairs (keys[i], i).  report (dict, optional) receives
    'heap_ranges': (first, last, has_ties) of every range that reached the depth limit."""
    n = len(keys)
    a = [(int(keys[i]), i) for i in range(n)]
    heaps, leaves = [], []
    stack = [(0, n, 2 * (n.bit_length() - 1))] if n > 1 else []
    while stack:
        f, l, d = stack.pop()
        while l - f > THRESHOLD:
            if d == 0:
                heaps.append((f, l, len({a[i][0] for i in range(f, l)}) < l - f))
                heap_sort(a, f, l)
                break
            d -= 1
            kk = [x[0] for x in a[f:l]]
            m = median_to_first(kk, 1, (l - f) // 2, l - f - 1)
            a[f], a[f + m] = a[f + m], a[f]
            kk[0], kk[m] = kk[m], kk[0]
            cut, swaps = partition_closed(kk, 0, l - f)
            for x, y in swaps:
                a[f + x], a[f + y] = a[f + y], a[f + x]
            stack.append((f + cut, l, d))
            l = f + cut
        else:
            leaves.append((f, l))
    for f, l in leaves:  # the final insertion pass: a stable sort inside every leaf
        a[f:l] = sorted(a[f:l], key=lambda t: t[0])
    if report is not None:
        report["heap_ranges"] = heaps
    return [i for _, i in a]


def voxel_pick(sorted_keys, sorted_idx):
    """VoxelMode::ANY: idx[start + (count*7 + start*13) % count] of every run of equal keys."""
    out, s, n = [], 0, len(sorted_keys)
    while s < n:
        e = s + 1
        while e < n and sorted_keys[e] == sorted_keys[s]:
            e += 1
        c = e - s
        out.append(sorted_idx[s + (c * 7 + s * 13) % c])
        s = e
    return out


def median3_killer(n):
    """Keys (0 .. n) on which std::sort reaches its depth limit with ties left in the heap-sorted range.
    McIlroy's adversary: values are decided only when a comparison needs them; a partition step made on undecided
    ("gas") elements freezes as few of them as it can.  The run stops at the first range that reaches the depth
    limit; every element still undecided then takes the largest key, so the heap range ends full of ties."""
    gas = n
    val = [gas] * n
    state = {"solid": 0, "cand": -1}

    def less(x, y):
        if val[x] == gas and val[y] == gas:
            z = x if x == state["cand"] else y
            val[z] = state["solid"]
            state["solid"] += 1
        if val[x] == gas:
            state["cand"] = x
        elif val[y] == gas:
            state["cand"] = y
        return val[x] < val[y]

    a = list(range(n))
    stack = [(0, n, 2 * (n.bit_length() - 1))]
    while stack:
        f, l, d = stack.pop()
        while l - f > THRESHOLD:
            if d == 0:
                return [val[i] for i in range(n)]
            d -= 1
            x, y, z = f + 1, f + (l - f) // 2, l - 1
            if less(a[x], a[y]):
                m = y if less(a[y], a[z]) else (z if less(a[x], a[z]) else x)
            elif less(a[x], a[z]):
                m = x
            else:
                m = z if less(a[y], a[z]) else y
            a[f], a[m] = a[m], a[f]
            first, last = f + 1, l
            while True:
                while less(a[first], a[f]):
                    first += 1
                last -= 1
                while less(a[f], a[last]):
                    last -= 1
                if not first < last:
                    break
                a[first], a[last] = a[last], a[first]
                first += 1
            stack.append((first, l, d))
            l = first
    return None


def _main():
    import random
    import numpy as np
    sys.path.insert(0, __file__.rsplit("/", 2)[0] + "/oracle")
    import fdm_ref_py as R
    R.load()
    rng = random.Random(7)
    for _ in range(20000):
        m = rng.randrange(17, 200)
        k = [rng.randrange(rng.choice([2, 5, 50])) for _ in range(m)]
        mp = median_to_first(k, 1, m // 2, m - 1)
        k[0], k[mp] = k[mp], k[0]
        assert partition_closed(k, 0, m) == partition_literal(k, 0, m)
    print("closed-form partition == literal loop on 20000 ranges")

    def check(base):
        x = np.asarray(base, dtype=np.float32) + np.float32(0.5)
        zero = np.zeros(len(base), dtype=np.float32)
        want = R.voxel_any(x, zero, zero, 1.0, stable=False)
        order = std_sort(base)
        return list(want) == voxel_pick([base[i] for i in order], order)

    cases = 0
    for trial in range(300):
        n = rng.choice([1, 2, 16, 17, 31, 33, 100, 1000, 3000])
        kind = trial % 5
        nv = rng.choice([1, 2, 3, 10, 1000])
        base = [rng.randrange(nv) for _ in range(n)]
        if kind == 1:
            base.sort()
        elif kind == 2:
            base.sort(reverse=True)
        elif kind == 3:
            base = [i % 2 for i in range(n)]
        elif kind == 4:
            base = [0] * n
        assert check(base), (n, kind)
        cases += 1
    print(f"model == oracle std::sort voxel picks on {cases} inputs")
    for n in (200, 2000, 5000):
        keys = median3_killer(n)
        rep = {}
        std_sort(keys, rep)
        assert any(t for _, _, t in rep["heap_ranges"]), n
        assert check(keys), n
        print(f"median-of-3 killer n={n}: heap ranges {[(f, l) for f, l, _ in rep['heap_ranges']]}, model == oracle")


if __name__ == "__main__":
    _main()
