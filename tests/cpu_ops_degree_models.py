"""The degree-sequence models restated in plain Python with unbounded ints, on top of ``cpu_ops_generative.word`` / ``below``: the
Erdös-Gallai condition in its textbook form, Havel-Hakimi as an independent second opinion, and the Molloy-Reed sampler of
``generative_models.molloy_reed`` — the keyed shuffle of the stubs, and the repair rounds with their claims, side bits and the
"not worse" acceptance rule — rule for rule as DESIGN.md ("Degree-sequence models") writes them down.  No numpy, no device."""
from cpu_ops_generative import below, stored, word

TAG_MR_SHUFFLE, TAG_MR_VICTIM, TAG_MR_SIDE = 6, 7, 8


def erdos_gallai(degrees) -> bool:
    """sum_{i <= r} d_i <= r (r - 1) + sum_{i > r} min(d_i, r) for r = 1 .. n on the descending sequence; no negative entry, an even sum."""
    d = sorted((int(x) for x in degrees), reverse=True)
    if any(x < 0 for x in d) or sum(d) % 2:
        return False
    return all(sum(d[:r]) <= r * (r - 1) + sum(min(x, r) for x in d[r:]) for r in range(1, len(d) + 1))


def havel_hakimi(degrees) -> bool:
    """Join the node of largest degree to the next largest ones, drop it, repeat: graphic iff this never runs out of partners."""
    d = sorted((int(x) for x in degrees), reverse=True)
    if any(x < 0 for x in d) or sum(d) % 2:
        return False
    while d and d[0] > 0:
        k, d = d[0], d[1:]
        if k > len(d) or d[k - 1] == 0:
            return False
        d = sorted([x - 1 for x in d[:k]] + d[k:], reverse=True)
    return True


def first_matching(degrees, seed):
    """The M = S / 2 oriented edges of the keyed shuffle: stubs sorted by (64-bit key, stub index), neighbours in that order are joined."""
    owner = [v for v, k in enumerate(degrees) for _ in range(int(k))]
    order = sorted(range(len(owner)), key=lambda s: (word(seed, TAG_MR_SHUFFLE, 0, s), s))
    pairs = [(owner[order[2 * i]], owner[order[2 * i + 1]]) for i in range(len(owner) // 2)]
    return [(min(u, w), max(u, w)) for u, w in pairs]


def sampler(degrees, seed, multiedge=False, relax=False, max_rounds=1 << 16, stats=None):
    """``(edges in edge order, repair rounds)``; ``stats`` (a dict) counts the claims that were blocked and the swaps proposed / accepted."""
    edges = first_matching(degrees, seed)
    M, rounds = len(edges), 0
    if relax:
        return edges, 0
    while True:
        by_key = sorted(range(M), key=lambda e: (edges[e], e))                    # the stable sort of (u n + w, e)
        flag = [0] * M
        for i, e in enumerate(by_key):
            loop = edges[e][0] == edges[e][1]
            surplus = not multiedge and i > 0 and edges[by_key[i - 1]] == edges[e]
            flag[e] = int(loop or surplus)
        offenders = [e for e in range(M) if flag[e]]
        if not offenders:
            return edges, rounds
        if rounds == max_rounds:
            raise RuntimeError("offenders left after the last round")
        rounds += 1
        present = set(edges)                                                        # the round-start snapshot of the keys
        victim = {e: below(M, seed, TAG_MR_VICTIM, rounds, e) for e in offenders}
        claim = {}
        for e, f in victim.items():
            claim[f] = min(claim.get(f, e), e)

        def bad(x):
            return int(x[0] == x[1] or (not multiedge and x in present))

        for e in offenders:
            f = victim[e]
            if f == e or claim[f] != e or e in claim:
                if stats is not None:
                    stats["blocked"] = stats.get("blocked", 0) + 1
                continue
            (a, b), (c, d) = edges[e], edges[f]
            if word(seed, TAG_MR_SIDE, rounds << 32, e) & 1:
                c, d = d, c
            e2, f2 = (min(a, c), max(a, c)), (min(b, d), max(b, d))
            new = bad(e2) + int(bad(f2) or (not multiedge and f2 == e2))
            if stats is not None:
                stats["proposed"] = stats.get("proposed", 0) + 1
            if new <= 1 + flag[f]:
                edges[e], edges[f] = e2, f2
                if stats is not None:
                    stats["accepted"] = stats.get("accepted", 0) + 1


def molloy_reed(degrees, seed, multiedge=False, relax=False):
    """``(stored pairs, repair rounds)`` of the package's graph: both directions; parallel edges kept with ``multiedge``; with ``relax`` the
    first matching with loops dropped and duplicates merged."""
    edges, rounds = sampler(degrees, seed, multiedge, relax)
    if relax:
        edges = [e for e in edges if e[0] != e[1]]
    return stored(edges, False, multi=multiedge and not relax), rounds
