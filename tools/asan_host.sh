#!/bin/bash
# The host side of the library (loaders, parsers, snapshot writer, BVH build, multi-device bookkeeping) under AddressSanitizer + UBSan, on the CPU:
# builds libngp_hip with -fsanitize=address,undefined for the HOST code only (-fno-gpu-sanitize: GPU sanitizers are not available on this pool) and
# runs the CPU tests against it through NGP_HIP_LIBRARY. The two tests that compile their own gcc-sanitized harnesses are left out (two sanitizer
# runtimes in one process tree do not mix); they run in the normal suite.
# usage: tools/asan_host.sh [pytest -k expression]
set -e
cd "$(dirname "$0")/.."
PKG=surface-irradiance-estimation-from-neural-radiance-fields_amd
OUT=${TMPDIR:-/tmp}/libngp_hip_asan.so
RT=$(/opt/rocm/lib/llvm/bin/clang -print-file-name=libclang_rt.asan-x86_64.so)
SOURCES=$(cd $PKG && python -B -c "import build; print(' '.join('csrc/' + s for s in build.SOURCES))") # the library's own source list
(cd $PKG && /opt/rocm/bin/hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -shared -ffp-contract=off -fno-slp-vectorize -fvisibility=hidden \
	-fsanitize=address,undefined -fno-sanitize=vptr,function -fno-gpu-sanitize -shared-libsan -o "$OUT" $SOURCES -lz 2>&1 | grep -v "warning\|^ \|generated" || true)
rm -f /tmp/asan_report* /tmp/ubsan_report*
LD_PRELOAD=$RT ASAN_OPTIONS=detect_leaks=0:log_path=/tmp/asan_report UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1:log_path=/tmp/ubsan_report NGP_HIP_LIBRARY=$OUT \
	python -m pytest tests/test_host_cpu.py -q -p no:cacheprovider -k "${1:-not parsers_survive and not image_decoders_survive}"
ls /tmp/asan_report* /tmp/ubsan_report* 2>/dev/null && { head -20 /tmp/asan_report* /tmp/ubsan_report*; exit 1; } || echo "no sanitizer report"
