"""No GPU: the replay schedule (``_graphs.run``) with counting stand-ins for the graphs, and the bounded cache that
keeps graph sets and loops (``_graphs.BoundedCache``)."""
import pytest

from sdfest_amd._graphs import BoundedCache, run


class _Graph:
    def __init__(self):
        self.replays = 0

    def replay(self):
        self.replays += 1


N_ITER = [0, 1, 4, 5, 6, 11]
PER_MANY = 5


@pytest.mark.parametrize("n_iter", N_ITER)
def test_run_replays_the_quotient_and_the_rest(n_iter):
    one, many = _Graph(), _Graph()
    run(n_iter, one, many, PER_MANY, None)
    assert (many.replays, one.replays) == (n_iter // PER_MANY, n_iter % PER_MANY)
    assert many.replays * PER_MANY + one.replays == n_iter


@pytest.mark.parametrize("n_iter", N_ITER)
def test_run_with_after_each_takes_the_one_iteration_graph_throughout(n_iter):
    one, many, seen = _Graph(), _Graph(), []
    # (after_each runs behind ITS iteration: as many replays as calls so far)
    run(n_iter, one, many, PER_MANY, None, after_each=lambda it: seen.append((it, one.replays)))
    assert (many.replays, one.replays) == (0, n_iter)
    assert seen == [(it, it + 1) for it in range(n_iter)]


@pytest.mark.parametrize("after", [False, True])
@pytest.mark.parametrize("n_iter", N_ITER)
def test_run_without_a_many_iteration_graph(n_iter, after):
    one, seen = _Graph(), []
    run(n_iter, one, None, PER_MANY, None, after_each=seen.append if after else None)
    assert one.replays == n_iter
    assert seen == (list(range(n_iter)) if after else [])


@pytest.mark.parametrize("after", [False, True])
@pytest.mark.parametrize("n_iter", N_ITER)
def test_run_eager(n_iter, after):
    """``use_graph=False``: no graph at all, every iteration is the eager callable"""
    calls, seen = [], []
    run(n_iter, None, None, PER_MANY, lambda: calls.append(len(calls)), after_each=seen.append if after else None)
    assert calls == list(range(n_iter))
    assert seen == (list(range(n_iter)) if after else [])


def test_bounded_cache_drops_the_oldest_inserted():
    cache = BoundedCache(4)
    for k in "abcd":
        cache[k] = k.upper()
    cache["a"] = "again"                    # an existing key: nothing leaves, and "a" stays the oldest
    assert len(cache) == 4 and list(cache) == list("abcd") and cache["a"] == "again"
    cache["e"] = "E"                        # the fifth new key
    assert len(cache) == 4 and "a" not in cache and list(cache) == list("bcde")
    assert cache.get("a") is None and cache.get("b") == "B" and list(cache.values()) == ["B", "C", "D", "E"]


def test_bounded_cache_get_or_build_builds_once():
    cache, built = BoundedCache(4), []

    def build():
        built.append(1)
        return None                         # (a stored None -- "cannot be built" -- counts as present)

    assert cache.get_or_build("k", build) is None and cache.get_or_build("k", build) is None
    assert built == [1] and "k" in cache
    for k in range(4):
        assert cache.get_or_build(k, lambda: k * k) == k * k
    assert list(cache) == [0, 1, 2, 3]      # "k" was the oldest
