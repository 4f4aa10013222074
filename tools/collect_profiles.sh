set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
if [ $# -ne 1 ] || [ -z "$1" ]; then echo "usage: bash tools/collect_profiles.sh OUTDIR (new or empty)" >&2; exit 2; fi
O=$(realpath -m "$1") || exit 2
if [ -e "$O" ] && [ -n "$(ls -A "$O")" ]; then echo "collect_profiles.sh: $O exists and is not empty" >&2; exit 1; fi
mkdir -p "$O"
cd "$R"
python tests/parity_report.py "$O"/parity.json > "$O"/parity.log 2>&1; tail -3 "$O"/parity.log | cut -c1-200
python bench.py --full > "$O"/bench_forward.json 2> "$O"/bench_forward.err; tail -1 "$O"/bench_forward.json | cut -c1-200
python bench.py --mode gradient --steps 3 --warmup 1 > "$O"/bench_gradient.json 2>/dev/null
python bench.py --grid 512 --nt 100 --steps 3 --warmup 1 --cpu-steps 0 > "$O"/bench_512.json 2>/dev/null; tail -1 "$O"/bench_512.json | cut -c60-140
cd /tmp && export TMPDIR=/tmp
timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d "$O"/kt256 -- python3 "$R"/bench.py --steps 2 --warmup 1 --cpu-steps 0 > /dev/null 2>&1
timeout -k 10 200 rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$O"/f256 -- python3 "$R"/bench.py --steps 1 --warmup 0 --nt 100 --cpu-steps 0 > /dev/null 2>&1
timeout -k 10 200 rocprofv3 --pmc WRITE_SIZE --output-format csv -d "$O"/w256 -- python3 "$R"/bench.py --steps 1 --warmup 0 --nt 100 --cpu-steps 0 > /dev/null 2>&1
timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d "$O"/kt512 -- python3 "$R"/bench.py --grid 512 --nt 60 --steps 2 --warmup 1 --cpu-steps 0 > /dev/null 2>&1
timeout -k 10 200 rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$O"/f512 -- python3 "$R"/bench.py --grid 512 --nt 30 --steps 1 --warmup 0 --cpu-steps 0 > /dev/null 2>&1
timeout -k 10 200 rocprofv3 --pmc WRITE_SIZE --output-format csv -d "$O"/w512 -- python3 "$R"/bench.py --grid 512 --nt 30 --steps 1 --warmup 0 --cpu-steps 0 > /dev/null 2>&1
timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d "$O"/ktgrad -- python3 "$R"/bench.py --mode gradient --steps 1 --warmup 1 > /dev/null 2>&1
cd "$R"; python tests/bench_mc.py --cpu-samples 100 > "$O"/mc.jsonl 2>/dev/null
ls "$O"/*/*/ | head -40
cd /tmp && timeout -k 10 120 rocprofv3 --kernel-trace --stats --output-format csv -d "$O"/kt2d -- python3 "$R"/tools/time_config.py --config cfg2 --nt 1000 --rounds 1 > "$O"/time2d.log 2>&1
cd "$R"
