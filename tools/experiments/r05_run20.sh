#!/bin/bash
# bw3 copy sweep + the default bench command (PMC child passes for C3 / C5 included), timed
out=${1:-out}      # output directory, relative to the repository root
mkdir -p $out
( while true; do date >> $out/r20_heartbeat.txt; sleep 45; done ) & HB=$!
timeout -k 10 300 tools/ubench/bw3 > $out/r20_bw3.txt 2>&1
tail -1 $out/r20_bw3.txt
t0=$(date +%s)
timeout -k 10 900 python bench.py --full > $out/r20_bench.json 2> $out/r20_bench.err
rc=$?
echo "bench rc=$rc wall=$(( $(date +%s) - t0 )) s"
kill $HB
exit $rc
