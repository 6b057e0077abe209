#!/bin/bash
# quick timing of the library's NT GEMM paths
export LD_LIBRARY_PATH=merlot_reserve_amd
timeout -k 10 200 scripts/micro/gemm3_test ${MODE:-quick} 6 || exit 1
