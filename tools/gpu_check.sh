#!/bin/bash
# full GPU test suite (+ optionally the full bench line), logs under $CHECK_OUT (default build/check/)
out=${CHECK_OUT:-build/check}
mkdir -p $out
python -m pytest tests -m gpu -x -q 2>&1 | tail -25 > $out/gputest.log
cat $out/gputest.log
if [ "$1" = "bench" ]; then
  python bench.py --full > $out/bench.json 2> $out/bench.err
  tail -c 6000 $out/bench.json
  tail -5 $out/bench.err
fi
