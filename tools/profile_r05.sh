# Round-5 profile pass (run on the GPU box through gpurun): the driver's bench form, rocprofv3 kernel stats in both stream
# modes, VALU / HBM counters of the C2 kernels (separate --pmc passes), the strong-scaling lines of config 5, the C4
# --second-best line with its kernel stats, two host threads per rank, the int16 multi-wave kernels.
# usage: bash tools/profile_r05.sh <tag>      -> gpurun_out/<tag>/...
V=${1:-r05}
export TMPDIR=/tmp
R=$PWD
O=$R/gpurun_out/$V
mkdir -p $O
python bench.py --full --steps 20 --warmup 3 > $O/bench_c2.json 2> $O/bench_c2.err
tail -c 200 $O/bench_c2.json; echo
python bench.py --full --steps 20 --warmup 3 --no-cpu-baseline --timed-only --host-threads 2 > $O/bench_c2_host_threads_2.json 2>/dev/null
(cd /tmp && rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats_c2 -o c2 -- python3 $R/bench.py --steps 20 --warmup 3 --no-cpu-baseline --timed-only > $O/stats_c2.log 2>&1)
(cd /tmp && rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats_c2_mode0 -o c2 -- python3 $R/bench.py --steps 10 --warmup 2 --no-cpu-baseline --timed-only --pipe-mode 0 > $O/stats_c2_mode0.log 2>&1)
(cd /tmp && rocprofv3 --pmc SQ_INSTS_VALU GRBM_GUI_ACTIVE --kernel-trace --output-format csv -d $O/pmc_valu_c2 -o p -- python3 $R/bench.py --steps 3 --warmup 1 --no-cpu-baseline --timed-only --pipe-mode 0 > $O/pmc_valu_c2.log 2>&1)
for c in FETCH_SIZE WRITE_SIZE; do (cd /tmp && rocprofv3 --pmc $c --kernel-trace --output-format csv -d $O/pmc_$c -o p -- python3 $R/bench.py --steps 3 --warmup 1 --no-cpu-baseline --timed-only --pipe-mode 0 > $O/pmc_$c.log 2>&1); done
python bench.py --full --config c5 --scaling strong --seq-len 25000000 --steps 10 --warmup 2 --no-cpu-baseline > $O/bench_c5_25mb.json 2>/dev/null
python bench.py --full --config c5 --scaling strong --steps 5 --warmup 1 --no-cpu-baseline > $O/bench_c5_200mb.json 2>/dev/null
python bench.py --full --config c4-second-best --steps 6 --warmup 2 > $O/bench_c4_second_best.json 2> $O/bench_c4_second_best.err
(cd /tmp && rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats_c4sb -o c4 -- python3 $R/bench.py --config c4-second-best --steps 4 --warmup 1 --no-cpu-baseline > $O/stats_c4sb.log 2>&1)
for m in 150 400; do for v in f16 i16; do if [ $v = i16 ]; then export SD_FILL_CELLS=i16; else unset SD_FILL_CELLS; fi; python bench.py --full --monomers $m --reads 128 --steps 3 --warmup 1 --no-cpu-baseline --timed-only --pipe-mode 0 2>/dev/null | python -c "import json,sys; j=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('monomers=$m', j['config']['cell_arithmetic'], 'ms/step', round(j['ms_per_step'],1), 'fill ms', round(j['kernel_ms_per_step']['fill'],1), 'Tcell/s', round(j['roofline']['cells_per_s']/1e12,2))"; done; done > $O/multiwave_i16.txt 2>&1
unset SD_FILL_CELLS
find $O -name "*.csv" | wc -l
