"""Brute-force PAM, written from the algorithm statement of DESIGN.md K11 alone; it shares no code
with consensus_clustering_amd/pam.py or the kernels.

SWAP recomputes the total deviation of every candidate medoid set outright, and every sum is
``math.fsum``, the exactly rounded sum, so a value does not depend on the order of its terms: two
candidates whose terms are the same numbers in another order (the two closest medoids at
K = m - 1 are the standing case: either may leave for the same total deviation; so are the two
equal row sums at m = 2) compare equal here, and the tie rule decides.

Next to the result the reference reports how close its decisions were.  ``margin`` is the
smallest relative difference between the value taken and the best value that differs from it
(BUILD: best against second best; SWAP: best pair against second best; and the smallest dTD
against 0), relative to the sums compared; ``ties`` counts the decisions whose runner-up has
exactly the value taken, which the tie rule settled and the margin leaves out.  An implementation
that adds in another order agrees with this one wherever the margin is well above m * 2^-52."""
import math
from collections import namedtuple

import numpy as np

Result = namedtuple("Result", "medoids labels inertia n_iter margin ties")


class _Margins:
    def __init__(self):
        self.margin, self.ties = math.inf, 0

    def decided(self, taken, others, scale):
        """One decision: the value taken, the values it beat, the size of the sums compared."""
        if any(v == taken for v in others):
            self.ties += 1
        differ = [abs(v - taken) for v in others if v != taken]
        if differ and scale > 0:  # against sums of 0 any difference is infinitely clear
            self.margin = min(self.margin, min(differ) / scale)


def total_deviation(D, medoids):
    return math.fsum(D[sorted(medoids)].min(axis=0))


def pam_ref(D, K, max_iter=300):
    D = np.asarray(D, dtype=np.float64)
    m = D.shape[0]
    note = _Margins()
    # BUILD
    sums = [math.fsum(D[i]) for i in range(m)]
    first = min(range(m), key=lambda i: (sums[i], i))
    note.decided(sums[first], sums[:first] + sums[first + 1:], abs(sums[first]))
    medoids = [first]
    near = D[first].copy()
    for _ in range(1, K):
        cand = [i for i in range(m) if i not in medoids]
        gains = [math.fsum(np.maximum(near - D[i], 0.0)) for i in cand]
        pos = min(range(len(cand)), key=lambda c: (-gains[c], cand[c]))
        note.decided(gains[pos], gains[:pos] + gains[pos + 1:], abs(gains[pos]))
        medoids.append(cand[pos])
        near = np.minimum(near, D[cand[pos]])
    # SWAP
    n_iter = 0
    while n_iter < max_iter:
        current = total_deviation(D, medoids)
        # every item's distance to the nearest medoid other than i: one half of the set less i plus h
        rest = {i: D[[x for x in medoids if x != i]].min(axis=0) if K > 1 else np.full(m, np.inf) for i in medoids}
        trials = []  # (total deviation, h, medoid item) in the order of the tie rule
        for h in range(m):
            if h in medoids:
                continue
            for i in sorted(medoids):
                trials.append((math.fsum(np.minimum(rest[i], D[h])), h, i))
        if not trials:
            break
        pos = min(range(len(trials)), key=lambda c: (trials[c][0], c))
        td, h, i = trials[pos]
        scale = max(current, td)
        note.decided(td, [t[0] for t in trials[:pos] + trials[pos + 1:]], scale)
        note.decided(td, [current], scale)  # dTD against 0
        if not td < current:
            break
        medoids[medoids.index(i)] = h
        n_iter += 1
    # labels
    medoids = sorted(medoids)
    labels = np.empty(m, dtype=np.int64)
    near = np.empty(m)
    for j in range(m):
        if j in medoids:
            labels[j] = medoids.index(j)
        else:
            labels[j] = min(range(K), key=lambda r: (D[medoids[r], j], r))
        near[j] = D[medoids[labels[j]], j]
    return Result(np.array(medoids), labels, math.fsum(near), n_iter, note.margin, note.ties)
