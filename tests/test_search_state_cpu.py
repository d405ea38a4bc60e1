"""SearchState, the host state of an IndexCorpus (core/search_engine.py), without a GPU: buffers, events and
streams are plain Python stand-ins handed to the state, which allocates nothing itself."""
import gc
import threading

from hq_mi355x.core.search_engine import _RING, IndexCorpus, SearchState, _RedoRing

KEY = ("cuda:0", 0)


class Buf:
    def __init__(self, dtype="int32"):
        self.dtype = dtype


class Event:
    """A timing event of `ms` milliseconds after the start event; done: what query() reports."""

    def __init__(self, ms=0.0, done=True):
        self.ms, self.done, self.waited = ms, done, False

    def query(self):
        return self.done

    def synchronize(self):
        self.waited = self.done = True

    def elapsed_time(self, end):
        assert end.done, "elapsed_time of a pair still running"
        return end.ms


class Batch:
    """Stand-in for a PendingSearch read on the side stream: it holds (ring, slot)."""

    def __init__(self, ring, slot):
        self.ring = (ring, slot)
        ring.unread[slot] = self


def _in_thread(fn):
    out = []
    th = threading.Thread(target=lambda: out.append(fn()))
    th.start()
    th.join()
    return out[0]


def test_ring_rotation():
    """40 takes: slots 0..15, 0..15, 0..7, each clearing the slot after it; a batch left unread in slot j comes
    back from the take about to clear j and from no other."""
    assert _RING == 16
    ring = _RedoRing(Buf())
    takes = [ring.take() for _ in range(40)]
    assert [t[0] for t in takes] == list(range(16)) * 2 + list(range(8))
    assert [t[1] for t in takes] == [(i + 1) % 16 for i in range(16)] * 2 + list(range(1, 9))
    assert all(t[2] is None for t in takes)
    assert ring.next == 8
    b = Batch(ring, 11)
    olds = [ring.take() for _ in range(16)]  # slots 8..15, 0..7: the take of slot 10 clears 11
    assert [(i, j) for i, j, old in olds if old is not None] == [(10, 11)]
    assert olds[2][2] is b
    ring.unread[11] = None  # read (IndexCorpus._resolve)
    assert all(ring.take()[2] is None for _ in range(16))


def test_threads_own_their_rings():
    """64 threads, one after the other, take the ring of one (device, stream): 64 distinct rings, none left
    after the last join, and the main thread's ring untouched.  Keyed by thread ident, as the rings were
    before SearchState, the threads here would have shared rings: idents are reused once a thread has ended."""
    st, other = SearchState(), SearchState()  # `other`: a corpus the main thread never searches
    made = []

    def make():
        made.append(Buf())
        return made[-1]

    def work():
        st.side(0, lambda: ("stream", Buf()))
        other.ring(KEY, Buf)
        other.side(0, lambda: ("stream", Buf()))
        return st.ring(KEY, make)

    mine = st.ring(KEY, make)
    st.side(0, lambda: ("stream", Buf()))
    seen = []
    for _ in range(64):
        r = _in_thread(work)
        assert r is not mine and r.next == 0 and r.unread == [None] * _RING
        seen.append(id(r.buf))  # the buffer stays referenced by `made`: its id cannot be reused
        del r
    assert len(set(seen)) == 64 and len(made) == 65
    gc.collect()
    assert other.live() == (0, 0)
    assert st.live() == (1, 1)  # the main thread's own
    assert st.ring(KEY, make) is mine and len(made) == 65


def test_ring_outlives_its_thread_while_a_batch_holds_it():
    """A batch submitted by a worker may be finished by another thread: its ring stays until the batch goes."""
    st = SearchState()

    def submit():
        ring = st.ring(KEY, Buf)
        i, _, _ = ring.take()
        return Batch(ring, i)

    b = _in_thread(submit)
    gc.collect()
    assert st.live() == (1, 0)
    ring, i = b.ring
    assert ring.unread[i] is b and st.ring(KEY, Buf) is not ring  # the finishing thread has a ring of its own
    del b, ring
    gc.collect()
    assert st.live() == (1, 0)  # this thread's, taken just above
    assert _in_thread(st.live) == (1, 0)


def test_finished_event_pairs_are_folded():
    """1000 redos whose events have completed: no pair is kept, dense_s is their sum in the order recorded."""
    st = SearchState()
    want = 0.0
    for k in range(1000):
        st.bump(redo_batches=1, events=(Event(), Event(ms=0.37 * k)))
        want += 0.37 * k / 1e3
        assert st.open_events == []
    assert st.dense_s == want
    s = st.stats()
    assert s["dense_s"] == want and s["redo_batches"] == 1000


def test_running_pairs_stay_open_until_stats():
    st = SearchState()
    pairs = [(Event(), Event(ms=2.0, done=False)) for _ in range(5)]
    for p in pairs:
        st.bump(redo_batches=1, redo_queries=3, events=p)
    st.bump(batches=1)  # no pair: nothing queried
    assert st.open_events == pairs and st.dense_s == 0.0
    pairs[1][1].done = True  # one ends: folded with the next redo, the others stay
    st.bump(events=(Event(), Event(ms=1.0)))
    assert st.open_events == pairs[:1] + pairs[2:] and st.dense_s == 2.0 / 1e3 + 1.0 / 1e3
    s = st.stats()
    assert all(e1.waited for k, (_, e1) in enumerate(pairs) if k != 1)
    waited = 0.0
    for _ in range(4):
        waited += 2.0 / 1e3
    assert s == dict(batches=1, queries=0, redo_batches=5, redo_queries=15, retry_queries=0, dense_queries=0,
                     dense_s=2.0 / 1e3 + 1.0 / 1e3 + waited)
    assert st.open_events == []
    st.bump(batches=1)
    assert s["batches"] == 1 and st.stats()["batches"] == 2  # a snapshot
    st.bump(events=(Event(), Event(ms=1.0, done=False)))
    st.reset_stats()
    assert st.open_events == [] and st.dense_s == 0.0
    assert st.stats() == dict(dict.fromkeys(SearchState.KEYS, 0), dense_s=0.0)


def test_counters_from_threads():
    st = SearchState()

    def work():
        for _ in range(1000):
            st.bump(batches=1, queries=16, dense_queries=2)

    ths = [threading.Thread(target=work) for _ in range(8)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    s = st.stats()
    assert (s["batches"], s["queries"], s["dense_queries"], s["retry_queries"]) == (8000, 128000, 16000, 0)


def test_list_lengths():
    st = SearchState()
    S = IndexCorpus.SLACK
    assert st.slack_for(20, S) == S and st.slack_for(100, S) == S
    st.adapt(20, 92)
    assert st.slack_for(20, S) == 92 and st.slack_for(100, S) == S
    st.reset_list_lengths()
    assert st.slack_for(20, S) == S


def test_pinned_pool():
    st = SearchState()
    made = []

    def make(dtype):
        made.append(Buf(dtype))
        return made[-1]

    a = st.pinned("int32", lambda: make("int32"))
    b = st.pinned("int32", lambda: make("int32"))
    assert a is not b and len(made) == 2
    st.unpin(a)
    c = st.pinned("bool", lambda: make("bool"))  # another dtype: the free int32 buffer is not for it
    assert c is made[2] and c.dtype == "bool"
    assert st.pinned("int32", lambda: make("int32")) is a and len(made) == 3
    st.unpin(c)
    st.unpin(b)
    assert st.pinned("bool", lambda: make("bool")) is c
    assert st.pinned("int32", lambda: make("int32")) is b
    assert st.pinned("int32", lambda: make("int32")) is made[3] and len(made) == 4


def test_fallback_slot_made_once_per_key():
    st = SearchState()
    calls = []
    a = st.fallback((16, "cuda:0", 0), lambda: calls.append(0) or ("best", "id", "det"))
    assert st.fallback((16, "cuda:0", 0), lambda: calls.append(0) or None) is a
    assert st.fallback((16, "cuda:0", 7), lambda: calls.append(0) or ("other",)) == ("other",)
    assert len(calls) == 2
