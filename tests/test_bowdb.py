"""DBoW2 score and KeyFrameDatabase, the parts that need no GPU: the CPU
restatement (tests/cpp/bowdb_ref.c) against an independent statement of each
scoring in exact rational arithmetic, the (smallest common word, add sequence)
order claim of orbv_db_query against the restatement's literal per-word lists,
and the host ASan/UBSan run of the store's bookkeeping
(csrc/bowdb_internal.h, tests/cpp/bowdb_main.cpp)."""
import numpy as np
import pytest

import bowdb_util as U
import native


@pytest.mark.parametrize("scoring", U.SCORINGS)
def test_restatement_equals_the_exact_statement(scoring):
    rng = np.random.default_rng(100 + scoring)
    nonzero = 0
    for trial in range(40):
        na, nb = int(rng.integers(0, 120)), int(rng.integers(0, 120))
        a = U.random_bow(rng, na, 300, signed=trial % 2 == 1)
        b = U.random_bow(rng, nb, 300, signed=trial % 2 == 1)
        want = U.exact_score(scoring, a, b)
        got = U.ref_score(scoring, a, b)
        assert got == want and np.signbit(got) == np.signbit(want), (trial, got, want)
        assert U.close(scoring, U.sum_forward(U.ref_terms(scoring, a, b))) == got
        nonzero += got != 0
    assert nonzero > 20
    for a, b in U.length_pairs()[:20]:
        assert U.ref_score(scoring, a, b) == U.exact_score(scoring, a, b)
    a, b = U.planted_order_pair(scoring)
    assert U.ref_score(scoring, a, b) == U.exact_score(scoring, a, b)


def test_chi_square_guard_in_the_restatement():
    a = U.bow([3, 8, 20], [0.5, 0.25, 0.125])
    b = U.bow([3, 8, 20], [0.5, -0.25, 0.375])
    # word 8: vi + wi == 0, no term (0 / 0 would be a NaN)
    assert len(U.ref_terms(2, a, b)) == 2
    assert U.ref_score(2, a, b) == 2.0 * (0.25 + 0.125 * 0.375 / 0.5)


def _sort_key_order(history, query):
    """the claim: sharing keyframes ordered by (smallest common word, add
    sequence), computed from the history alone"""
    seq, live = 0, {}
    for op, kid, b in history:
        if op == "add":
            live[kid] = (seq, b)
            seq += 1
        else:
            live.pop(kid, None)
    rows = []
    for kid, (s, (w, _)) in live.items():
        c = np.intersect1d(w, query[0])
        if len(c):
            rows.append((int(c[0]), s, kid, len(c)))
    rows.sort()
    return [r[2] for r in rows], [r[3] for r in rows]


@pytest.mark.parametrize("seed", range(6))
def test_order_is_smallest_common_word_then_add_sequence(seed):
    rng = np.random.default_rng(seed)
    db, history, present = U.RefDb(200, 0), [], []
    regrouped = 0
    for step in range(160):
        r = rng.uniform()
        if present and r < 0.3:
            kid = present.pop(int(rng.integers(len(present))))
            db.erase(kid)
            history.append(("erase", kid, None))
            if rng.uniform() < 0.5:  # and again, with the same id: to the back
                b = U.random_bow(rng, 12, 200)
                db.add(kid, b)
                history.append(("add", kid, b))
                present.append(kid)
                regrouped += 1
        elif r < 0.35:
            db.erase(10 ** 6 + step)  # absent
            history.append(("erase", 10 ** 6 + step, None))
        else:
            b = U.random_bow(rng, int(rng.integers(0, 16)), 200)
            db.add(step, b)
            history.append(("add", step, b))
            present.append(step)
        if step % 20 == 19:
            q = U.random_bow(rng, 15, 200)
            ids, nc, _ = db.query(q)
            want_ids, want_nc = _sort_key_order(history, q)
            assert ids.tolist() == want_ids and nc.tolist() == want_nc
    assert regrouped > 5 and db.size() == len(present)
    # not vacuous: ties on the smallest common word exist and add order decides them
    q = U.random_bow(rng, 15, 200)
    ids, _, _ = db.query(q)
    assert len(ids) > 10 and ids.tolist() != sorted(ids.tolist())
    db.clear()
    assert db.size() == 0 and len(db.query(q)[0]) == 0


def test_store_bookkeeping_clean_under_asan_ubsan():
    r = native.run_sanitized("bowdb_main")
    assert "0 failures" in r.stdout
