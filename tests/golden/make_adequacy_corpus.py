"""Generate tests/golden/adequacy/n{2,3,4,5,8}.json: the parity inputs that tell every oracle
mutant (tests/adequacy.py MUTANTS) apart from the checker, at every CACHE_SIZE class.

TEST INFRASTRUCTURE (uses the oracle and its mutant builds only; the project's own data).

Per node count N:
  * the candidates 0..POOL[N]-1 of adequacy.candidates(N, .) -- small systems (2 or 4 blocks, 1..N
    homes, at most 24 instructions per node), each with a 64-bit schedule seed -- are run under the
    checker and under every mutant, at every CACHE_SIZE of adequacy.CACHE_SIZES, all-lockstep and
    under their own seeds. A candidate whose checker run has a queue deeper than 16 or raises
    ROUNDCAP / STUCK / OVERFLOW anywhere is dropped (the corpus must stay in the first queue tier);
  * a greedy set cover picks at most 256 candidates so that every (mutant, CACHE_SIZE, evaluation)
    cell is told apart by at least 3 of them. At N >= 3 a cell left short is an error. At N = 2 a
    short cell goes to `exempt` with the number of candidates searched and found; every
    candidate found is in the corpus;
  * micro-step section: candidates in order, each with a walk seed and per-node weights for
    orc_random_walk (STRICT model); at most 32 are picked so that every mutant is told apart by
    at least one walk at CACHE_SIZE 1, 4 and 3 (adequacy.micro_kills).
The files record the candidate ids; fixture_from_ids() rebuilds a file from its ids alone (the
CPU test compares that with the committed file), a full run of this script redoes the search.

Run: python tests/golden/make_adequacy_corpus.py [N ...]   (about a minute per node count)
"""
import json
import pathlib
import sys

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import adequacy as ad  # noqa: E402

POOL = {2: 51200, 3: 16384, 4: 16384, 5: 16384, 8: 16384}
MICRO_POOL = 8192
EVALS = ("lockstep", "seeded")


def hex_rows(tr, lens):
    return ["".join(f"{int(w):04x}" for w in tr[t, :int(lens[t])]) for t in range(len(lens))]


def fixture_from_ids(N, ids, micro_ids, exempt, pool):
    packed, lens, seeds, _, _ = ad.candidates(N, ids)
    mp, ml, _, wseeds, weights = ad.candidates(N, micro_ids)
    out = {"source": "tests/golden/make_adequacy_corpus.py (candidates of tests/adequacy.py; rows: one hex string "
                     "per node, 4 digits per packed instruction)",
           "num_procs": N, "candidates_searched": pool,
           "systems": [{"cand": int(i), "seed": f"{int(seeds[k]):016x}", "rows": hex_rows(packed[k], lens[k])}
                       for k, i in enumerate(ids)],
           "micro": [{"cand": int(i), "walk_seed": f"{int(wseeds[k]):016x}", "weights": [int(w) for w in weights[k]],
                      "rows": hex_rows(mp[k], ml[k])} for k, i in enumerate(micro_ids)]}
    if N == 2:
        out["exempt"] = exempt
    return out


def dumps(fx):
    return json.dumps(fx, indent=1).replace("\n   ", " ").replace("\n  }", " }") + "\n"


def search(N):
    pool = POOL[N]
    packed, lens, seeds, wseeds, weights = ad.candidates(N, np.arange(pool))
    muts = sorted(ad.MUTANTS)
    cells = [(k, CS, ev) for CS in ad.CACHE_SIZES for ev in range(2) for k in muts]
    K = np.zeros((len(cells), pool), bool)
    valid = np.ones(pool, bool)
    for CS in ad.CACHE_SIZES:
        for ev in range(2):
            sd = seeds if ev else None
            base = ad.run_many(ad.lib(0), packed, lens, N, CS, sd)
            valid &= (base[1] <= 16) & ((base[2] & ad.BAD_ERRORS) == 0)
            for k in muts:
                K[cells.index((k, CS, ev))] = ad.kills(ad.lib(k), packed, lens, N, CS, sd, base)
    K &= valid
    chosen, left = ad.greedy_cover(K, ad.MIN_KILLS, ad.MAX_SYSTEMS)
    if left:
        raise SystemExit(f"N={N}: {ad.MAX_SYSTEMS} systems do not cover cells {[cells[c] for c in left]}")
    exempt = []
    for c in np.flatnonzero(K.sum(axis=1) < ad.MIN_KILLS):  # the pool itself is short: greedy took all it has
        k, CS, ev = cells[c]
        found = np.flatnonzero(K[c]).tolist()
        if N != 2 or not set(found) <= set(chosen):
            raise SystemExit(f"N={N}: cell m{k} CACHE_SIZE {CS} {EVALS[ev]} short ({len(found)} found) and not exemptible")
        exempt.append({"mutant": k, "cache_size": CS, "evaluation": EVALS[ev], "searched": pool,
                       "found": len(found), "systems": sorted(chosen.index(f) for f in found)})
    ids = sorted(chosen)
    for e in exempt:  # positions in the sorted corpus
        e["systems"] = sorted(ids.index(chosen[p]) for p in e["systems"])

    # micro-step section: walks of the checker, replayed under every mutant
    # (every mutant for the first 1024 candidates, then only those still not told apart)
    mcells = [(k, CS) for CS in ad.MICRO_CS for k in muts]
    limit = pool if N == 2 else MICRO_POOL
    MK = np.zeros((len(mcells), limit), bool)
    open_cells = set(mcells)
    searched = 0
    for c in range(limit):
        if c >= 1024 and not open_cells:
            break
        searched = c + 1
        walks = [ad.walk(packed[c], lens[c], N, CS, int(wseeds[c]), weights[c]) for CS in ad.MICRO_CS]
        if any(w is None for w in walks):
            continue
        for j, CS in enumerate(ad.MICRO_CS):
            ks = [k for k in muts if c < 1024 or (k, CS) in open_cells]
            if not ks:
                continue
            want = ad.replay(ad.lib(0), packed[c], lens[c], N, CS, walks[j][1])
            for k in ks:
                if ad.replay(ad.lib(k), packed[c], lens[c], N, CS, walks[j][1]) != want:
                    MK[mcells.index((k, CS)), c] = True
                    open_cells.discard((k, CS))
    mchosen, left = ad.greedy_cover(MK, 1, ad.MAX_MICRO)
    if left:
        raise SystemExit(f"N={N}: {ad.MAX_MICRO} walks do not cover micro cells {[mcells[c] for c in left]}")
    for k, CS in sorted(open_cells):
        if N != 2:
            raise SystemExit(f"N={N}: micro cell m{k} CACHE_SIZE {CS} not covered")
        exempt.append({"mutant": k, "cache_size": CS, "evaluation": "micro", "searched": searched, "found": 0,
                       "systems": []})
    return fixture_from_ids(N, ids, sorted(mchosen), exempt, pool)


if __name__ == "__main__":
    (HERE / "adequacy").mkdir(exist_ok=True)
    for N in [int(a) for a in sys.argv[1:]] or ad.NODE_COUNTS:
        fx = search(N)
        text = dumps(fx)
        (HERE / "adequacy" / f"n{N}.json").write_text(text)
        print(f"n{N}.json: {len(fx['systems'])} systems, {len(fx['micro'])} micro, {len(fx.get('exempt', []))} exempt, "
              f"{len(text)} bytes", flush=True)
