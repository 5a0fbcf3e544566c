#!/bin/bash
# Full GPU validation of the tree: pytest -m gpu, smoke(), default bench line.
set -o pipefail
mkdir -p bench_out
timeout -k 10 900 python -u -m pytest tests -m gpu -q --timeout 300 --timeout-method thread -p no:cacheprovider > bench_out/full_pytest.log 2>&1
echo "pytest rc=$?"; tail -3 bench_out/full_pytest.log; grep -E "FAILED|ERROR" bench_out/full_pytest.log | head -20
timeout -k 10 200 python -c "import __graft_entry__ as g; g.smoke()" > bench_out/full_smoke.log 2>&1
echo "smoke rc=$?"; tail -2 bench_out/full_smoke.log
timeout -k 10 400 python bench.py --full > bench_out/full_bench.json 2> bench_out/full_bench.err
echo "bench rc=$?"
python3 -c "import json;d=json.loads(open('bench_out/full_bench.json').read().strip().splitlines()[-1]);print(d['value'], d['ms_per_step'], d['roofline']['frac'], d['roofline_gae']['us_per_launch'], d['roofline_gae_65536']['exact']['frac'], d['cpu_baseline']['value'])"
