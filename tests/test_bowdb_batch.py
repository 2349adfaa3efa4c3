"""The batched keyframe-database queries, the parts that need no GPU: the host
ASan/UBSan run of the CSR / word validation, the word gate and the offset
packing (csrc/bowdb_internal.h, tests/cpp/bowdb_batch_main.cpp), and the claim
the order kernel rests on, against the restatement's literal per-word lists:
sorting a query's sharing keyframes by (rank of the smallest common word in the
query, add position) reproduces the list."""
import numpy as np
import pytest

import bowdb_util as U
import native
import test_bowdb as B  # the histories' order statement, imported and not edited


def test_batch_host_pieces_clean_under_asan_ubsan():
    r = native.run_sanitized("bowdb_batch_main")
    assert "0 failures" in r.stdout


def _rank_order(history, query):
    """sharing keyframes by (rank in the query of the smallest common word, add
    position), from the history alone; the rank is an index into the query,
    never a word id"""
    pos, live = 0, {}
    for op, kid, b in history:
        if op == "add":
            live[kid] = (pos, b)
            pos += 1
        else:
            live.pop(kid, None)
    qw = query[0].tolist()
    rows = []
    for kid, (at, (w, _)) in live.items():
        hit = np.isin(query[0], w)
        if hit.any():
            rank = int(np.argmax(hit))
            assert qw[rank] in w.tolist() and not np.isin(query[0][:rank], w).any()
            rows.append((rank, at, kid, int(hit.sum())))
    rows.sort()
    return [r[2] for r in rows], [r[3] for r in rows], [r[0] for r in rows]


@pytest.mark.parametrize("seed", range(6))
def test_rank_then_add_position_reproduces_the_list(seed):
    """the histories of test_bowdb.test_order_is_smallest_common_word_then_add_sequence"""
    rng = np.random.default_rng(seed)
    db, history, present = U.RefDb(200, 0), [], []
    ties = spread = checked = 0
    for step in range(160):
        r = rng.uniform()
        if present and r < 0.3:
            kid = present.pop(int(rng.integers(len(present))))
            db.erase(kid)
            history.append(("erase", kid, None))
            if rng.uniform() < 0.5:
                b = U.random_bow(rng, 12, 200)
                db.add(kid, b)
                history.append(("add", kid, b))
                present.append(kid)
        elif r < 0.35:
            db.erase(10 ** 6 + step)
            history.append(("erase", 10 ** 6 + step, None))
        else:
            b = U.random_bow(rng, int(rng.integers(0, 16)), 200)
            db.add(step, b)
            history.append(("add", step, b))
            present.append(step)
        if step % 20 == 19:
            q = U.random_bow(rng, 15, 200)
            ids, nc, _ = db.query(q)
            want_ids, want_nc, ranks = _rank_order(history, q)
            assert ids.tolist() == want_ids and nc.tolist() == want_nc
            # ... and it is the order test_bowdb states with the word itself as the key
            assert B._sort_key_order(history, q) == (want_ids, want_nc)
            assert all(0 <= r < 15 for r in ranks)
            ties += len(ranks) - len(set(ranks))
            spread = max(spread, len(set(ranks)))
            checked += 1
    assert checked == 8 and ties > 5 and spread >= 5  # bins with several entries, and several bins
