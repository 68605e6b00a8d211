# Repository-level targets.  `python __graft_entry__.py` (build()) is what the driver runs; these are conveniences.
PKG = 3d-gaussian-splatting-for-novel-view-synthesis_amd
ASAN_DIR = build/asan
ASAN_FLAGS = -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined

all:
	python __graft_entry__.py

# Sanitizers run on the CPU builds only (GPU AddressSanitizer is not available on the pool): the host build of the projection
# math (the same gs_math.h / gs_body.h the HIP kernels inline) and the plain-C oracle, each under AddressSanitizer + UBSan,
# driven by their own test files.  Python is not instrumented, so the runtime is preloaded and leak checking is off.
# The MCMC arithmetic (gs_mcmc.h), the 3D filter (gs_filter3d.h), the exposure transform (gs_exposure.h), the bilateral grid (gs_bilagrid.h), the image metrics (gs_metrics.h), the nearest-neighbour search (gs_knn.h) and the pose corrections (gs_pose_delta.h) go through stand-alone instrumented programs of their own, which
# need no preloaded runtime.
check-asan: check-asan-mcmc check-asan-filter3d check-asan-exposure check-asan-bilagrid check-asan-metrics check-asan-knn check-asan-pose_delta
	mkdir -p $(ASAN_DIR)
	g++ $(ASAN_FLAGS) -std=c++17 -shared -fPIC -o $(ASAN_DIR)/libgsmath_host_asan.so $(PKG)/csrc/host_math_check.cpp
	gcc $(ASAN_FLAGS) -std=c99 -fopenmp -shared -fPIC -o $(ASAN_DIR)/libgs_oracle_asan.so oracle/gs_oracle.c -lm
	LD_PRELOAD="$$(gcc -print-file-name=libasan.so) $$(gcc -print-file-name=libubsan.so)" ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 \
	  UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 OMP_NUM_THREADS=4 \
	  GSPLAT_HOSTMATH_LIB=$(CURDIR)/$(ASAN_DIR)/libgsmath_host_asan.so GS_ORACLE_LIB=$(CURDIR)/$(ASAN_DIR)/libgs_oracle_asan.so \
	  python -m pytest tests/test_product_math_cpu.py tests/test_pose_grad_cpu.py tests/test_c_oracle_golden.py -x -q -p no:cacheprovider

check-asan-metrics: SELFTEST_FLAGS = -ffp-contract=off
check-asan-knn: SELFTEST_FLAGS = -ffp-contract=off
check-asan-%: $(PKG)/csrc/host_%_selftest.cpp
	mkdir -p $(ASAN_DIR)
	g++ $(ASAN_FLAGS) $(SELFTEST_FLAGS) -std=c++17 -o $(ASAN_DIR)/host_$*_selftest $<
	ASAN_OPTIONS=halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 $(ASAN_DIR)/host_$*_selftest

# (the check-asan-% targets are not listed: make skips the pattern-rule search for a phony target; they name no file, so they always run)
.PHONY: all check-asan
