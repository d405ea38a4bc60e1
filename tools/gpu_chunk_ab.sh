#!/bin/bash
# cfg5 chunk encoder: parity tests, then the stream leg of the bench (kernel time under rocprof)
export TMPDIR=/tmp
OUT=${OUT:-prof_out}
mkdir -p $OUT
if [ -z "$NO_TESTS" ]; then
timeout -k 10 600 python -u -m pytest $(grep -ln "chunk_encode" tests/test_gpu_*.py) -q -x --timeout 500 --timeout-method thread > $OUT/chunk_t.log 2>&1
rc=$?; echo "tests rc=$rc"; tail -3 $OUT/chunk_t.log
[ $rc -eq 0 ] || exit $rc
fi
for spec in "$@"; do
  opts=""; for o in ${spec//,/ }; do [ "$o" != "default" ] && opts="$opts --option $o"; done
  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/cab -o run --output-format csv -- python3 bench.py --full --steps 2 --warmup 1 --n-emb 10000 --no-cpu --no-search --no-precomputed --no-ingest --no-frames $opts > $OUT/cab.log 2>&1
  rc=$?; [ $rc -eq 0 ] || { echo "$spec rc=$rc"; tail -3 $OUT/cab.log; exit $rc; }
  echo "[$spec] $(python3 tools/prof_summary.py $OUT/cab | grep -E 'k_chunk_np' | tr -s ' ' | cut -c1-100) $(grep -o '"stream": {"metric[^}]*' $OUT/cab.log | grep -o '"value": [0-9.]*')"
done
