"""The one capture-and-replay path of the captured loops (``pipeline.py``, ``init_network.py``): warm-up, capture
and state restore (``capture``), the replay schedule of a run (``run``) and the bounded caches that keep graphs and
loops (``BoundedCache``)."""
import torch


def capture(device, sequences, warmup, state=(), **graph_kwargs):
    """One new ``torch.cuda.CUDAGraph`` per callable of `sequences`, in order, each with its own memory pool.
    `warmup()` runs first, on a fresh side stream (lazy module loads must not happen under capture); the tensors of
    `state` are put back to what they held on entry after the warm-up and after the captures (a capture does not
    execute, but keep the state explicit) -- also when the warm-up or a capture raises: the exception propagates and no
    graph is handed out, so a caller that assigns its graphs from the return value is left as it was.
    graph_kwargs go to ``torch.cuda.graph`` (``capture_error_mode=``)."""
    saved = [t.clone() for t in state]

    def restore():
        for t, c in zip(state, saved):
            t.copy_(c)

    try:
        side = torch.cuda.Stream(device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            warmup()
        torch.cuda.current_stream(device).wait_stream(side)
        restore()
        graphs = []
        for sequence in sequences:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, **graph_kwargs):
                sequence()
            graphs.append(graph)
    finally:
        restore()
    return graphs


def run(n_iter, one, many, per_many, eager, after_each=None):
    """`n_iter` iterations: `many` (a graph of `per_many` iterations, or None) for the quotient, then iteration by
    iteration -- `one.replay()`, or `eager()` where `one` is None.  `after_each(it)` (`it`: the iteration's index in the
    run) has to see every iteration, so with it all of them take the one-iteration path."""
    done = 0
    if many is not None and after_each is None:
        for _ in range(n_iter // per_many):
            many.replay()
        done = n_iter - n_iter % per_many
    step = eager if one is None else one.replay
    for it in range(done, n_iter):
        step()
        if after_each is not None:
            after_each(it)


class BoundedCache(dict):
    """A dict of at most `limit` entries: a new key at the limit drops the oldest-inserted entry first (a caller whose
    key changes from call to call re-builds instead of collecting graphs and buffers without bound)."""

    def __init__(self, limit):
        super().__init__()
        self.limit = limit

    def __setitem__(self, key, value):
        if key not in self and len(self) >= self.limit:
            del self[next(iter(self))]
        super().__setitem__(key, value)

    def get_or_build(self, key, build):
        if key not in self:
            self[key] = build()
        return self[key]
