"""Argument checks of the search library's re-rank and corpus-mutation entries, pinned call by call: a table of
calls with deliberately bad (or empty) arguments against the return code and hq_last_error text the library gave
before the host layer was folded into one check path.  Every call returns before any HIP call (no launch, no
memset), so no GPU is needed and the pointers are never read: non-null ones are made-up addresses."""
import pytest

OK, INVALID, UNSUPPORTED = 0, -1, -5
P, P2 = 0x1000, 0x2000  # made-up non-null addresses
BIG = 0x7FFFFFFF        # the first row count past the int32 row ids

# A valid call of each entry, by argument name in the C order (include/hq_mi355x.h); a case overrides some.
_REFINE_HEAD = dict(Rq=P, Zq=P, Sq=P, Q=4, Rc=P, Zc=P, Sc=P, N=100, L=64, mode=0, cand_score=P, cand_id=P, kp=28, k=20,
                    threshold=0.0, thr_mode=0, eps=1e-9, id_base=0, out_score=P, out_id=P, out_count=P, out_resolved=P,
                    count_empty=0, out_redo=None)
_SPLIT = dict(Z16=None, S32=None, Zov16=None, Sov32=None, flags=None)
ENTRIES = {
    "hq_refine_topk": dict(_REFINE_HEAD, stream=None),
    "hq_refine_rescore_topk": dict(_REFINE_HEAD, out_det=P, stream=None),
    "hq_refine_rescore_topk_pp": dict(_REFINE_HEAD, out_redo=P, next_redo=P2, out_det=P, stream=None),
    "hq_refine_topk_ws": dict(_REFINE_HEAD, next_redo=None, out_det=None, workspace=None, workspace_bytes=0,
                              stream=None),
    "hq_refine_final_ws": dict({k: v for k, v in _REFINE_HEAD.items() if k not in ("mode", "count_empty")},
                               next_redo=None, K_out=10, fin_id=P, fin_det=P, fin_count=P, workspace=None,
                               workspace_bytes=0, stream=None),
    "hq_seg_append": dict(idx=P, M=3, L=64, src_f32=0, row_f32=None, N0=10, Z=P, stats=P, **_SPLIT, stream=None),
    "hq_seg_gather": dict(src_row=P, M=3, N_src=10, L=64, R_src=P, Z_src=P, S_src=P, R=P2, Z=P2, stats=P2, **_SPLIT,
                          stream=None),
    "hq_seg_replace": dict(idx=P, M=3, rows=P, L=64, src_f32=0, row_f32=None, N=10, Z=P, stats=P, **_SPLIT,
                           stream=None),
    "hq_seg_prepare_pack0": dict(idx=P, N=3, L=64, src_f32=0, row_f32=None, Z=P, stats=P, Z16=P, S32=P, stream=None),
}
_NULL_REFINE = dict(Rq=None, Zq=None, Sq=None, Rc=None, Zc=None, Sc=None, cand_score=None, cand_id=None,
                    out_score=None, out_id=None, out_count=None, out_resolved=None)
_ALL_NULL = {
    "hq_refine_topk": dict(_NULL_REFINE, Q=0),
    "hq_refine_rescore_topk": dict(_NULL_REFINE, Q=0, out_det=None),
    "hq_refine_rescore_topk_pp": dict(_NULL_REFINE, Q=0, out_det=None, out_redo=None, next_redo=None),
    "hq_refine_topk_ws": dict(_NULL_REFINE, Q=0),
    "hq_refine_final_ws": dict(_NULL_REFINE, Q=0, fin_id=None, fin_det=None, fin_count=None),
    "hq_seg_append": dict(M=0, idx=None, Z=None, stats=None),
    "hq_seg_gather": dict(M=0, N_src=0, src_row=None, R_src=None, Z_src=None, S_src=None, R=None, Z=None, stats=None),
    "hq_seg_replace": dict(M=0, idx=None, rows=None, Z=None, stats=None),
}

NULL = "null buffer"
PAIR = "a split copy needs both of its buffers"
FLAGS = "the flagged-row list needs the level-0 copies"
NOSEG = "no level structure for L=1"
LEVEL0 = "level-0 copies with a level-0 segment of 64 values"
NOOV = "overall copies without a split overall layout (L=128)"
WS = "workspace too small"

# (entry, overrides of the valid call, return code, hq_last_error text or None for a success)
CASES = [
    # ---- hq_refine_topk: sizes, the common buffers, Q = 0
    ("hq_refine_topk", dict(kp=0, k=0), INVALID, "bad sizes kp=0 k=0"),
    ("hq_refine_topk", dict(k=29), INVALID, "bad sizes kp=28 k=29"),
    ("hq_refine_topk", dict(k=0), INVALID, "bad sizes kp=28 k=0"),
    ("hq_refine_topk", dict(kp=1025, k=20), INVALID, "bad sizes kp=1025 k=20"),
    ("hq_refine_topk", dict(Q=-1), INVALID, "bad sizes kp=28 k=20"),
    ("hq_refine_topk", dict(N=-1), INVALID, "bad sizes kp=28 k=20"),
    ("hq_refine_topk", dict(L=0), INVALID, "bad sizes kp=28 k=20"),
    ("hq_refine_topk", _NULL_REFINE, INVALID, NULL),
    ("hq_refine_topk", dict(Rq=None), INVALID, NULL),
    ("hq_refine_topk", dict(Zq=None), INVALID, NULL),
    ("hq_refine_topk", dict(Sq=None), INVALID, NULL),
    ("hq_refine_topk", dict(cand_score=None), INVALID, NULL),
    ("hq_refine_topk", dict(cand_id=None), INVALID, NULL),
    ("hq_refine_topk", dict(out_score=None), INVALID, NULL),
    ("hq_refine_topk", dict(out_id=None), INVALID, NULL),
    ("hq_refine_topk", dict(out_score=None, out_id=None), INVALID, NULL),
    ("hq_refine_topk", dict(out_count=None), INVALID, NULL),
    ("hq_refine_topk", dict(out_resolved=None), INVALID, NULL),
    ("hq_refine_topk", dict(Rc=None), INVALID, NULL),
    ("hq_refine_topk", dict(Zc=None), INVALID, NULL),
    ("hq_refine_topk", dict(Sc=None), INVALID, NULL),
    ("hq_refine_topk", _ALL_NULL["hq_refine_topk"], OK, None),
    ("hq_refine_topk", dict(_ALL_NULL["hq_refine_topk"], kp=0), INVALID, "bad sizes kp=0 k=20"),  # sizes come first
    # ---- hq_refine_rescore_topk: also the records
    ("hq_refine_rescore_topk", dict(kp=0, k=0), INVALID, "bad sizes kp=0 k=0"),
    ("hq_refine_rescore_topk", dict(out_det=None), INVALID, NULL),
    ("hq_refine_rescore_topk", dict(out_id=None), INVALID, NULL),
    ("hq_refine_rescore_topk", dict(Sc=None), INVALID, NULL),
    ("hq_refine_rescore_topk", _ALL_NULL["hq_refine_rescore_topk"], OK, None),
    # ---- hq_refine_rescore_topk_pp: the records and both counters, which differ
    ("hq_refine_rescore_topk_pp", dict(kp=65, k=66), INVALID, "bad sizes kp=65 k=66"),
    ("hq_refine_rescore_topk_pp", dict(out_det=None), INVALID, NULL),
    ("hq_refine_rescore_topk_pp", dict(out_redo=None), INVALID, NULL),
    ("hq_refine_rescore_topk_pp", dict(next_redo=None), INVALID, NULL),
    ("hq_refine_rescore_topk_pp", dict(out_redo=P, next_redo=P), INVALID, NULL),
    ("hq_refine_rescore_topk_pp", dict(out_count=None), INVALID, NULL),
    ("hq_refine_rescore_topk_pp", _ALL_NULL["hq_refine_rescore_topk_pp"], OK, None),
    # ---- hq_refine_topk_ws: out_redo only together with next_redo; the workspace size
    ("hq_refine_topk_ws", dict(kp=0, k=0), INVALID, "bad sizes kp=0 k=0"),
    ("hq_refine_topk_ws", dict(out_score=None), INVALID, NULL),
    ("hq_refine_topk_ws", dict(next_redo=P2, out_redo=None), INVALID, NULL),
    ("hq_refine_topk_ws", dict(next_redo=P, out_redo=P), INVALID, NULL),
    ("hq_refine_topk_ws", dict(kp=108, k=100, workspace=P, workspace_bytes=64), INVALID, WS),
    ("hq_refine_topk_ws", dict(workspace=P, workspace_bytes=0), INVALID, WS),  # also where no kernel would use it
    ("hq_refine_topk_ws", dict(kp=108, k=100, workspace=P, workspace_bytes=64, Rq=None), INVALID, NULL),
    ("hq_refine_topk_ws", _ALL_NULL["hq_refine_topk_ws"], OK, None),
    # ---- hq_refine_final_ws: K_out, a cooperative shape (before Q = 0), optional lists, the final outputs
    ("hq_refine_final_ws", dict(kp=0, k=0), INVALID, "bad sizes kp=0 k=0 K=10"),
    ("hq_refine_final_ws", dict(K_out=0), INVALID, "bad sizes kp=28 k=20 K=0"),
    ("hq_refine_final_ws", dict(L=63, K_out=0), INVALID, "bad sizes kp=28 k=20 K=0"),
    ("hq_refine_final_ws", dict(L=63), UNSUPPORTED, "fused final ranking: kp=28 L=63"),
    ("hq_refine_final_ws", dict(L=63, kp=108, k=100, workspace=P, workspace_bytes=1 << 30), UNSUPPORTED,
     "fused final ranking: kp=108 L=63"),
    ("hq_refine_final_ws", dict(L=256), UNSUPPORTED, "fused final ranking: kp=28 L=256"),
    ("hq_refine_final_ws", dict(Q=65536, kp=108, k=100, workspace=P, workspace_bytes=1 << 40), UNSUPPORTED,
     "fused final ranking: kp=108 L=64"),
    ("hq_refine_final_ws", dict(_ALL_NULL["hq_refine_final_ws"], L=63), UNSUPPORTED, "fused final ranking: kp=28 L=63"),
    ("hq_refine_final_ws", _ALL_NULL["hq_refine_final_ws"], OK, None),
    ("hq_refine_final_ws", dict(_ALL_NULL["hq_refine_final_ws"], kp=108, k=100), OK, None),
    ("hq_refine_final_ws", dict(out_score=None), INVALID, NULL),
    ("hq_refine_final_ws", dict(out_id=None), INVALID, NULL),
    ("hq_refine_final_ws", dict(out_score=None, out_id=None, out_count=None), INVALID, NULL),
    ("hq_refine_final_ws", dict(fin_id=None), INVALID, NULL),
    ("hq_refine_final_ws", dict(fin_det=None), INVALID, NULL),
    ("hq_refine_final_ws", dict(fin_count=None), INVALID, NULL),
    ("hq_refine_final_ws", dict(Rc=None), INVALID, NULL),
    ("hq_refine_final_ws", dict(next_redo=P2, out_redo=None), INVALID, NULL),
    ("hq_refine_final_ws", dict(next_redo=P, out_redo=P), INVALID, NULL),
    ("hq_refine_final_ws", dict(kp=108, k=100), INVALID, NULL),  # long lists need the workspace
    ("hq_refine_final_ws", dict(kp=108, k=100, workspace=P, workspace_bytes=64), INVALID, WS),
    # ---- hq_seg_append
    ("hq_seg_append", dict(L=0), INVALID, "bad shape N0=10 M=3 L=0"),
    ("hq_seg_append", dict(M=-1), INVALID, "bad shape N0=10 M=-1 L=64"),
    ("hq_seg_append", dict(N0=-1), INVALID, "bad shape N0=-1 M=3 L=64"),
    ("hq_seg_append", dict(L=5000), UNSUPPORTED, "L=5000 (<= 4096)"),
    ("hq_seg_append", _ALL_NULL["hq_seg_append"], OK, None),
    ("hq_seg_append", dict(idx=None), INVALID, NULL),
    ("hq_seg_append", dict(Z=None), INVALID, NULL),
    ("hq_seg_append", dict(stats=None), INVALID, NULL),
    ("hq_seg_append", dict(Z16=P), INVALID, PAIR),
    ("hq_seg_append", dict(S32=P), INVALID, PAIR),
    ("hq_seg_append", dict(Zov16=P), INVALID, PAIR),
    ("hq_seg_append", dict(Sov32=P), INVALID, PAIR),
    ("hq_seg_append", dict(flags=P), INVALID, FLAGS),
    ("hq_seg_append", dict(flags=P, Zov16=P, Sov32=P), INVALID, FLAGS),
    ("hq_seg_append", dict(N0=BIG - 3), UNSUPPORTED, "N=2147483647 rows (int32 row ids)"),
    ("hq_seg_append", dict(N0=BIG - 3, Z16=P), INVALID, PAIR),  # the pointer tests come before the row limit
    ("hq_seg_append", dict(N0=BIG - 3, L=1), UNSUPPORTED, "N=2147483647 rows (int32 row ids)"),  # the shape tests after
    ("hq_seg_append", dict(L=1), INVALID, NOSEG),
    ("hq_seg_append", dict(L=128, Z16=P, S32=P), INVALID, LEVEL0),
    ("hq_seg_append", dict(L=128, Zov16=P, Sov32=P), INVALID, NOOV),
    # ---- hq_seg_gather
    ("hq_seg_gather", dict(L=0), INVALID, "bad shape N_src=10 M=3 L=0"),
    ("hq_seg_gather", dict(M=-1), INVALID, "bad shape N_src=10 M=-1 L=64"),
    ("hq_seg_gather", dict(N_src=0), INVALID, "bad shape N_src=0 M=3 L=64"),
    ("hq_seg_gather", dict(M=BIG), UNSUPPORTED, "M=2147483647 rows (int32 row ids)"),
    ("hq_seg_gather", _ALL_NULL["hq_seg_gather"], OK, None),
    ("hq_seg_gather", dict(src_row=None), INVALID, NULL),
    ("hq_seg_gather", dict(Z_src=None), INVALID, NULL),
    ("hq_seg_gather", dict(S_src=None), INVALID, NULL),
    ("hq_seg_gather", dict(Z=None), INVALID, NULL),
    ("hq_seg_gather", dict(stats=None), INVALID, NULL),
    ("hq_seg_gather", dict(R_src=None), INVALID, "the raw rows need both of their buffers"),
    ("hq_seg_gather", dict(R=None), INVALID, "the raw rows need both of their buffers"),
    ("hq_seg_gather", dict(Z16=P), INVALID, PAIR),
    ("hq_seg_gather", dict(Sov32=P), INVALID, PAIR),
    ("hq_seg_gather", dict(flags=P), INVALID, FLAGS),
    ("hq_seg_gather", dict(L=1), INVALID, NOSEG),
    ("hq_seg_gather", dict(L=128, Z16=P, S32=P), INVALID, LEVEL0),
    ("hq_seg_gather", dict(L=128, Zov16=P, Sov32=P), INVALID, NOOV),
    ("hq_seg_gather", dict(R=P), INVALID, "a destination buffer is its source"),
    ("hq_seg_gather", dict(Z=P), INVALID, "a destination buffer is its source"),
    ("hq_seg_gather", dict(stats=P), INVALID, "a destination buffer is its source"),
    ("hq_seg_gather", dict(Z=P, L=1), INVALID, NOSEG),  # the layout tests come before that one
    # ---- hq_seg_replace
    ("hq_seg_replace", dict(L=0), INVALID, "bad shape N=10 M=3 L=0"),
    ("hq_seg_replace", dict(M=11), INVALID, "bad shape N=10 M=11 L=64"),
    ("hq_seg_replace", dict(N=-1, M=0), INVALID, "bad shape N=-1 M=0 L=64"),
    ("hq_seg_replace", dict(L=5000), UNSUPPORTED, "L=5000 (<= 4096)"),
    ("hq_seg_replace", _ALL_NULL["hq_seg_replace"], OK, None),
    ("hq_seg_replace", dict(idx=None), INVALID, NULL),
    ("hq_seg_replace", dict(rows=None), INVALID, NULL),
    ("hq_seg_replace", dict(Z=None), INVALID, NULL),
    ("hq_seg_replace", dict(stats=None), INVALID, NULL),
    ("hq_seg_replace", dict(S32=P), INVALID, PAIR),
    ("hq_seg_replace", dict(Zov16=P), INVALID, PAIR),
    ("hq_seg_replace", dict(flags=P), INVALID, FLAGS),
    ("hq_seg_replace", dict(N=BIG), UNSUPPORTED, "N=2147483647 rows (int32 row ids)"),
    ("hq_seg_replace", dict(N=BIG, S32=P), INVALID, PAIR),
    ("hq_seg_replace", dict(N=BIG, L=1), UNSUPPORTED, "N=2147483647 rows (int32 row ids)"),
    ("hq_seg_replace", dict(L=1), INVALID, NOSEG),
    ("hq_seg_replace", dict(L=128, Z16=P, S32=P), INVALID, LEVEL0),
    ("hq_seg_replace", dict(L=128, Zov16=P, Sov32=P), INVALID, NOOV),
    # ---- hq_seg_prepare_pack0 (its copies are not optional)
    ("hq_seg_prepare_pack0", dict(L=0), INVALID, "bad shape N=3 L=0"),
    ("hq_seg_prepare_pack0", dict(N=-1), INVALID, "bad shape N=-1 L=64"),
    ("hq_seg_prepare_pack0", dict(idx=None), INVALID, NULL),
    ("hq_seg_prepare_pack0", dict(Z=None), INVALID, NULL),
    ("hq_seg_prepare_pack0", dict(stats=None), INVALID, NULL),
    ("hq_seg_prepare_pack0", dict(Z16=None), INVALID, NULL),
    ("hq_seg_prepare_pack0", dict(S32=None), INVALID, NULL),
    ("hq_seg_prepare_pack0", dict(N=0, idx=None, Z=None, stats=None, Z16=None), INVALID, NULL),
    ("hq_seg_prepare_pack0", dict(L=1), INVALID, NOSEG),
    ("hq_seg_prepare_pack0", dict(L=128), UNSUPPORTED, "level-0 segment of 64 values (<= 32)"),
    ("hq_seg_prepare_pack0", dict(L=5000), UNSUPPORTED, "level-0 segment of 1024 values (<= 32)"),
]


def _args(entry, over):
    unknown = set(over) - set(ENTRIES[entry])
    assert not unknown, f"{entry} has no argument {sorted(unknown)}"
    return tuple(dict(ENTRIES[entry], **over).values())


@pytest.fixture(scope="module")
def lib():
    from hq_mi355x import _lib
    return _lib.load()


def test_table_matches_the_signatures():
    from hq_mi355x._lib import SIGNATURES
    for entry, names in ENTRIES.items():
        assert len(names) == len(SIGNATURES[entry][1]), entry
    assert {c[0] for c in CASES} == set(ENTRIES)
    # every case ends in the argument checks: it is an error, or an empty problem with nothing to clear
    for entry, over, rc, msg in CASES:
        a = dict(ENTRIES[entry], **over)
        assert (rc != OK) == (msg is not None)
        assert rc != OK or (a.get("Q", 1) == 0 or a.get("M", 1) == 0) and a.get("next_redo") is None, (entry, over)


@pytest.mark.parametrize("case", range(len(CASES)), ids=lambda i: f"{CASES[i][0]}-{i}")
def test_argument_check(lib, case):
    from hq_mi355x import _lib
    entry, over, rc, msg = CASES[case]
    assert getattr(lib, entry)(*_args(entry, over)) == rc
    if rc != OK:  # hq_last_error keeps a stale text after a success
        assert _lib.last_error() == msg
