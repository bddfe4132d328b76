# GPU-side command list behind profiles/rNN_vMM_*: tests, smoke, bench line (--full), rocprofv3 kernel stats of the profile workload and of
# bench.py --full itself (without the 2M-observation K1 launches: the stats file averages over all launches of a kernel name), Cholesky timings,
# per-config baseline table.  Run from anywhere on the GPU host:  bash tools/refresh_profiles.sh r02_v21 [out-dir]  (results in out-dir/r02_v21,
# default profile_runs/ at the repository root)
set -x
V=$1
R=$(cd "$(dirname "$0")/.." && pwd)
O=$(mkdir -p "${2:-$R/profile_runs}/$V" && cd "${2:-$R/profile_runs}/$V" && pwd)
cd $R
timeout 1200 python -m pytest tests -m gpu -q 2>&1 | tail -8 > $O/pytest_gpu.txt
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -1 > $O/smoke.txt
timeout 600 python bench.py --full > $O/bench.json 2> $O/bench.err
cd /tmp && export TMPDIR=/tmp
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_w -- python $R/tools/profile_workload.py all > /tmp/prof_w.log 2>&1
cp $(find /tmp/prof_w -name "*kernel_stats.csv" | head -1) $O/kernel_stats.csv
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_n -- python $R/tools/profile_workload.py band > /tmp/prof_n.log 2>&1
cp $(find /tmp/prof_n -name "*kernel_stats.csv" | head -1) $O/band_kernel_stats.csv; tail -1 /tmp/prof_n.log > $O/band_workload.txt
timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_b -- python $R/bench.py --full --no-beyond-l3 --no-cpu-baseline > /tmp/prof_b.log 2>&1
cp $(find /tmp/prof_b -name "*kernel_stats.csv" | head -1) $O/bench_py_kernel_stats.csv
tail -1 /tmp/prof_b.log > $O/bench_under_rocprof.json
cd $R; cat $O/pytest_gpu.txt $O/smoke.txt; head -c 600 $O/bench.json
PYTHONPATH=$R python $R/tools/chol_time.py > $O/chol_time.txt 2>&1; cat $O/chol_time.txt
PYTHONPATH=$R timeout 600 python $R/tools/baseline_table.py > $O/baseline_table.md 2> $O/baseline_table.err; cat $O/baseline_table.md
