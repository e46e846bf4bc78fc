"""No GPU: the order-free contract pair_choice_kernel is written to (tests/pair_choice_model.py: contract -- the header of
csrc/pair_device.h restated from sets) is sound with respect to the reference's loop (literal: ScoreBuffer::top1PE as written).

For every generated pair the kernels may decide themselves (not `host`) the literal loop runs over several candidate orders and several
running means:
  * not tied  -> every evaluation gives the same found / winners / insert size, and no "equal" pair is counted: the kernel may settle it;
  * tied, not dup -> no "equal" pair is counted anywhere, and wherever exactly one best-scoring combination is closest to the running
    mean that combination wins in every order: what closed_between in the select stage (csrc/mapper_select.cpp) relies on.
The same generator feeds tests/test_gpu_pair_choice.py; its coverage of the edges it is there for is asserted here, before any GPU sees it."""
import numpy as np
import pytest

import pair_choice_model as M


@pytest.fixture(scope="module")
def batches():
    out = M.make_batches()
    return [(bt, [M.contract(bt, p) for p in range(bt.n_pairs)]) for bt in out]


def _orders(rng, c):
    ident = np.arange(c)
    return [ident, ident[::-1]] + [rng.permutation(c) for _ in range(4)]


def test_contract_is_sound_for_every_order_and_running_mean(batches):
    rng = np.random.default_rng(5)
    checked = {"settled": 0, "tied": 0, "unique closest": 0, "choice": 0, "skipped": 0}
    for bt, cons in batches:
        assert bt.min_d >= 0
        for p, c in enumerate(cons):
            if c.cls == "empty" or c.host:
                continue
            choice = c.cls != "simple"
            checked["choice"] += choice
            if c.n_combo > M.LITERAL_LIMIT:
                checked["skipped"] += choice
                continue
            if c.tied and c.dup:
                continue   # the candidate order decides: nothing is promised
            means = {0, 1, 10 ** 9}
            for d in {t[0] for t in c.tops}:
                means |= {d - 1, d, d + 1}
            ca, cb = bt.mate(p, 0)[1], bt.mate(p, 1)[1]
            outcomes = {}
            for oa, ob in zip(_orders(rng, ca), _orders(rng, cb)):
                (ps, d, a, b), mq_a, mq_b = M.literal_walk(bt, p, oa, ob)
                assert (mq_a, mq_b) == (c.mq_a, c.mq_b), (bt.name, bt.tags[p])
                assert len(ps) == c.n_combo, (bt.name, bt.tags[p])
                for avg in means:
                    outcomes.setdefault(avg, set()).add(tuple(M.check_pairs_loop(ps, d, a, b, avg)))
            for avg, got in outcomes.items():
                assert {g[0] for g in got} == {int(c.found)}, (bt.name, bt.tags[p], avg, got)
                assert {g[3] for g in got} == {0}, (bt.name, bt.tags[p], avg, got)   # `equal`
            if not c.tied:
                everything = set().union(*outcomes.values())
                assert len(everything) == 1, (bt.name, bt.tags[p], everything)
                if c.found:
                    (f, wa, wb, eq, dist), = everything
                    assert c.tops == {(dist, wa, wb)}
                checked["settled"] += 1
            else:
                checked["tied"] += 1
                for avg, got in outcomes.items():
                    if not c.found:
                        continue
                    far = sorted((abs(t[0] - avg), t) for t in c.tops)
                    if len(far) == 1 or far[0][0] < far[1][0]:
                        t = far[0][1]
                        assert got == {(1, t[1], t[2], 0, t[0])}, (bt.name, bt.tags[p], avg, got, t)
                        checked["unique closest"] += 1
    assert checked["settled"] > 5000 and checked["tied"] > 500 and checked["unique closest"] > 2000, checked
    assert checked["skipped"] < 0.05 * checked["choice"], checked


def test_generator_reaches_the_edges_it_names(batches):
    """what the GPU test relies on: the model finds, among the generated pairs, every class the kernels treat differently"""
    bt, cons = batches[0]
    per_class = {k: sum(1 for c in cons if c.cls == k) for k in ("empty", "simple", "small", "large")}
    assert per_class["small"] > 8192 and per_class["large"] > 1024 and sum(c.huge for c in cons) > 256, per_class   # persistent loops
    every = [c for _, cs in batches for c in cs]
    choice = [c for c in every if c.cls in ("small", "large")]
    live = [c for c in choice if not c.host]
    assert {0, 1, 63, 64, 65} <= {c.n_combo for c in live}
    assert {1, 2, 8, 9} <= {c.n_top for c in live}
    assert {2047, 2048, 2049, 8192, 8193} <= {max(c.n_above) for c in choice}
    assert {2047, 2048, 2049} <= {min(c.n_above) for c in choice}   # on both sides
    counts = {(bt.mate(p, 0)[1], bt.mate(p, 1)[1]) for bt, cs in batches for p in range(bt.n_pairs)}
    assert {(1, 2), (2, 1), (2, 2), (63, 1), (64, 1), (65, 1), (1, 64), (1, 65), (64, 64), (65, 65), (64, 65), (256, 1), (257, 2), (300, 3), (65536, 1), (2, 65536), (65535, 1),
            (0, 0), (0, 1), (1, 0), (0, 70), (70, 0)} <= counts
    for want in ({"found": True, "tied": False}, {"found": False, "tied": False, "n_combo": 0}, {"found": False, "tied": True}, {"found": True, "tied": True, "dup": False},
                 {"found": True, "tied": True, "dup": True, "n_combo": 65}, {"found": False, "tied": True, "dup": True}):
        for cls in ("small", "large"):
            assert any(all(getattr(c, k) == v for k, v in want.items()) for c in live if c.cls == cls), (cls, want)
    assert any(c.huge and not c.host and c.found and c.n_combo > 64 for c in choice) and any(c.huge and c.host for c in choice)
    assert any(c.huge and not c.host and c.n_combo == 0 for c in choice) and any(c.huge and not c.host and not c.tied and c.found for c in choice)
    assert any(c.host and not c.huge for c in choice)
    # ties below the top only: tied, exactly one best-scoring combination
    assert any(c.tied and not c.dup and c.n_top == 1 for c in live) and any(c.tied and c.dup and c.n_top == 1 and c.n_combo <= 64 for c in live)
    # the strict window bounds, in every batch, on one-candidate pairs and on pairs with choices: a combination exactly at min, min + 1,
    # max - 1 and max; the `int` that wraps (out of the window, and into it); two mates at one location
    for bt, cs in batches:
        for classes in (("simple",), ("small", "large")):
            reached = set().union(*(c.edges for c in cs if c.cls in classes and not c.host))
            assert {"min", "min+1", "max-1", "max", "wrap", "wrap into the window", "same location"} <= reached, (bt.name, classes, reached)
    # ... and at those bounds the loop itself takes the pair or does not: what the tags promise is what the literal model sees
    for bt, cs in batches:
        for p, c in enumerate(cs):
            if bt.tags[p].startswith("bound 1x1 d="):
                assert c.cls == "simple" and M.literal(bt, p)[0] == int(bt.tags[p].endswith(("min+1", "max-1"))), (bt.name, bt.tags[p])
    # the insert sizes of the settled one-candidate pairs without an upper bound reach 2^30 and beyond
    bt, cons = batches[3]
    assert bt.max_insert == 0
    sizes = {M.literal(bt, p)[4] for p, c in enumerate(cons) if c.cls == "simple" and c.found}
    assert {2 ** 30 - 1, 2 ** 30, 2 ** 30 + 1, 2 ** 31 - 2} <= sizes
