# One GPU session (it works from the repo root, wherever it is started): parity tests,
# smoke, the full bench line, rocprofv3 kernel-trace summaries of the same bench
# (parent, and the co-resident xGMI children per pid), and the two PMC passes
# (FETCH_SIZE, WRITE_SIZE) that give HBM traffic.  Every GPU step has its own
# time limit; the script stops at the first step that faults, aborts or times
# out.  Outputs land in $OUT (default session_out/; copied to profiles/ afterwards).
# SKIP_TESTS=1 skips the parity tests (a measurement-only session).
cd "$(dirname "$0")/.." || exit 1
OUT="${OUT:-session_out}"
mkdir -p "$OUT"
export TMPDIR=/tmp
rc=0
if [ -z "$SKIP_TESTS" ]; then
  timeout -k 10 900 python -u -m pytest tests -m gpu -q -p no:cacheprovider --timeout 400 --timeout-method thread > "$OUT/pytest_gpu.log" 2>&1
  rc=$?; echo "pytest rc=$rc" >> "$OUT/pytest_gpu.log"
  if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
fi
timeout -k 10 120 python -u -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1 || exit $?
timeout -k 10 600 python -u bench.py --full > "$OUT/bench.log" 2>&1 || exit $?
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof" -o bench_%pid% -- python3 bench.py --full --no-cpu-baseline --no-host-fed --no-tcp-edge --sweep-mib "" > "$OUT/prof.log" 2>&1 || exit $?
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$OUT/pmc_fetch" -o run -- python3 bench.py --full --steps 10 --warmup 2 --no-cpu-baseline --no-host-fed --no-tcp-edge --xgmi-coresident 0 > "$OUT/pmc_fetch.log" 2>&1 || exit $?
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --output-format csv -d "$OUT/pmc_write" -o run -- python3 bench.py --full --steps 10 --warmup 2 --no-cpu-baseline --no-host-fed --no-tcp-edge --xgmi-coresident 0 > "$OUT/pmc_write.log" 2>&1 || exit $?
python3 tools/pmc_summary.py --fetch "$OUT/pmc_fetch" --write "$OUT/pmc_write" --elems 67108864 --commit "${ONO_COMMIT:-unknown}" --session "${ONO_SESSION:-gpu_session.sh}" --out "$OUT/pmc_n1.json" > "$OUT/pmc_summary.log" 2>&1
exit $rc
