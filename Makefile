# Build the product library (HIP, gfx950) and the CPU oracle (test infrastructure).
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
# -structurizecfg-skip-uniform-regions: uniform branches stay plain scalar branches (no i1 flow masks in
# SGPR pairs): row kernel 4.70 -> 4.21 ms per 512 1080p pictures (tools/ab_libs2.sh, round 3)
# Do not add -ffp-contract=fast (here or through `make variant FLAGS=`): resize_math.h's rs_norm keeps its fp32 multiply
# and add apart with `#pragma clang fp contract(off)`, which hipcc's default fast-honor-pragmas respects and `fast` overrides
HIPFLAGS ?= -O3 -std=c++17 --offload-arch=$(ARCH) -fPIC -shared -Wall -Wno-unused-function -mllvm -structurizecfg-skip-uniform-regions=true
# (sparse_host.cpp, upload_host.cpp: the host-only parts of the upload, plain C++ -- see sparse-check, upload-check;
# export_host.cpp, resize_host.cpp: the host-only parts of the device-side output and its scaled form;
# pichash_host.cpp: the picture hash of a host plane; grid_host.cpp, grid_resize_host.cpp: the host-only parts of the
# grid export and its scaled, ragged form)
SRC := p265_amd/csrc/p265r.hip p265_amd/csrc/sparse_host.cpp p265_amd/csrc/upload_host.cpp p265_amd/csrc/export_host.cpp \
       p265_amd/csrc/pichash_host.cpp p265_amd/csrc/resize_host.cpp p265_amd/csrc/grid_host.cpp \
       p265_amd/csrc/grid_resize_host.cpp
HDR := $(wildcard p265_amd/csrc/*.h) include/p265r.h

CXX ?= g++
FESRC := $(wildcard p265_amd/csrc/fe/*.cpp)
FEHDR := $(wildcard p265_amd/csrc/fe/*.h) include/p265fe.h include/p265r.h

# negative-test builds of the half-CTU publish self-checks (tests/test_a_multirank.py): prep places the
# publish point one job early, with (1) and without (2) prep's own check; and the two A/B phase schedules
# of a pipelined context (tests/test_gpu_parity.py, per-run digests)
CHECKVARIANTS := p265_amd/libp265r_brbroken1.so p265_amd/libp265r_brbroken2.so \
                 p265_amd/libp265r_phaseorder.so p265_amd/libp265r_earlyres.so

all: p265_amd/libp265r.so p265_amd/libp265fe.so p265_amd/libp265probe.so $(CHECKVARIANTS) oracle

p265_amd/libp265r_brbroken%.so: $(SRC) $(HDR)
	$(HIPCC) $(HIPFLAGS) -DP265R_BR_BROKEN=$* -o $@ $(SRC)

p265_amd/libp265r_phaseorder.so: $(SRC) $(HDR)
	$(HIPCC) $(HIPFLAGS) -DP265R_PHASE_ORDER=1 -o $@ $(SRC)

p265_amd/libp265r_earlyres.so: $(SRC) $(HDR)
	$(HIPCC) $(HIPFLAGS) -DP265R_EARLY_RESIDUAL=1 -o $@ $(SRC)

# measurement helper (not the product path): the row kernel's job-loop issue ceiling (bench.py)
p265_amd/libp265probe.so: p265_amd/csrc/issue_probe.hip
	$(HIPCC) -O3 -std=c++17 --offload-arch=$(ARCH) -fPIC -shared -Wall -o $@ $<

# native syntax front-end (host C++, no GPU code)
p265_amd/libp265fe.so: $(FESRC) $(FEHDR)
	$(CXX) -O3 -std=c++17 -fPIC -shared -pthread -Wall -Wextra -Wno-unused-parameter -o $@ $(FESRC)

p265_amd/libp265r.so: $(SRC) $(HDR)
	$(HIPCC) $(HIPFLAGS) -o $@ $(SRC)

oracle:
	$(MAKE) -C oracle

clean:
	rm -f p265_amd/libp265r.so p265_amd/libp265fe.so p265_amd/libp265probe.so $(CHECKVARIANTS) tools/sparse_check tools/upload_check tools/export_check tools/hash_check tools/mono_check tools/resize_check tools/prep_check tools/grid_check tools/grid_resize_check
	$(MAKE) -C oracle clean

.PHONY: all oracle clean

# host sanitizer check of the sparse upload's host code (sparsify + record validation, malformed inputs
# included): a stand-alone CPU program, not part of `all`
sparse-check: tools/sparse_check.cpp p265_amd/csrc/sparse_host.cpp p265_amd/csrc/sparse_host.h include/p265r.h
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=all \
		-o tools/sparse_check tools/sparse_check.cpp p265_amd/csrc/sparse_host.cpp
	./tools/sparse_check
.PHONY: sparse-check

# host sanitizer check of the upload's planner and packer (layout, chunk copy lists, staged bytes, rejection
# codes): a stand-alone CPU program, not part of `all`
upload-check: tools/upload_check.cpp p265_amd/csrc/upload_host.cpp p265_amd/csrc/sparse_host.cpp \
              p265_amd/csrc/upload_host.h p265_amd/csrc/sparse_host.h p265_amd/csrc/batch_types.h include/p265r.h
	$(CXX) -O1 -g -std=c++17 -pthread -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=all \
		-o tools/upload_check tools/upload_check.cpp p265_amd/csrc/upload_host.cpp p265_amd/csrc/sparse_host.cpp
	./tools/upload_check
.PHONY: upload-check

# host sanitizer check of the device-side output's host code (descriptor validation, layout, slot checks, RGB
# coefficients): a stand-alone CPU program, not part of `all`
export-check: tools/export_check.cpp p265_amd/csrc/export_host.cpp p265_amd/csrc/export_host.h include/p265r.h
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=all \
		-o tools/export_check tools/export_check.cpp p265_amd/csrc/export_host.cpp
	./tools/export_check
.PHONY: export-check

# host sanitizer check of the monochrome (chroma_format_idc 0) forms: the upload's planner, packer and validation
# for pictures without chroma (malformed ones included) and the one-plane export layouts: a stand-alone CPU program,
# not part of `all`
mono-check: tools/mono_check.cpp p265_amd/csrc/upload_host.cpp p265_amd/csrc/sparse_host.cpp p265_amd/csrc/export_host.cpp \
            p265_amd/csrc/upload_host.h p265_amd/csrc/sparse_host.h p265_amd/csrc/export_host.h p265_amd/csrc/batch_types.h include/p265r.h
	$(CXX) -O1 -g -std=c++17 -pthread -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=all \
		-o tools/mono_check tools/mono_check.cpp p265_amd/csrc/upload_host.cpp p265_amd/csrc/sparse_host.cpp p265_amd/csrc/export_host.cpp
	./tools/mono_check
.PHONY: mono-check

# host sanitizer check of the picture hash arithmetic (pichash_math.h through p265r_plane_hash_host: RFC 1321's
# vectors, the CRC and checksum split forms against restatements of D.3.19, rejection codes): a stand-alone CPU
# program, not part of `all`
hash-check: tools/hash_check.cpp p265_amd/csrc/pichash_host.cpp p265_amd/csrc/pichash_math.h include/p265r.h
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=all \
		-o tools/hash_check tools/hash_check.cpp p265_amd/csrc/pichash_host.cpp
	./tools/hash_check
.PHONY: hash-check

# host sanitizer check of the scaled device-side output's host code (resize_math.h through resize_plane_host against a
# brute-force restatement, the reciprocal division, malformed descriptors): a stand-alone CPU program, not part of `all`
resize-check: tools/resize_check.cpp p265_amd/csrc/resize_host.cpp p265_amd/csrc/export_host.cpp p265_amd/csrc/resize_host.h \
              p265_amd/csrc/resize_math.h p265_amd/csrc/export_host.h include/p265r.h
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=all \
		-o tools/resize_check tools/resize_check.cpp p265_amd/csrc/resize_host.cpp p265_amd/csrc/export_host.cpp
	./tools/resize_check
.PHONY: resize-check

# host sanitizer check of the grid export's host code (every refusal, the window, the oriented layout at the size
# extremes): a stand-alone CPU program, not part of `all`
grid-check: tools/grid_check.cpp p265_amd/csrc/grid_host.cpp p265_amd/csrc/export_host.cpp p265_amd/csrc/grid_host.h \
            p265_amd/csrc/export_host.h include/p265r.h
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=all \
		-o tools/grid_check tools/grid_check.cpp p265_amd/csrc/grid_host.cpp p265_amd/csrc/export_host.cpp
	./tools/grid_check
.PHONY: grid-check

# host sanitizer check of the scaled grid export's host code (every refusal, the per-frame constants against a
# restatement of the orientation rule, the tile-width reciprocal at every step): a stand-alone CPU program, not part
# of `all`
GRID_RESIZE_CHECK ?= tools/grid_resize_check
grid-resize-check: tools/grid_resize_check.cpp p265_amd/csrc/grid_resize_host.cpp p265_amd/csrc/grid_host.cpp \
                   p265_amd/csrc/resize_host.cpp p265_amd/csrc/export_host.cpp p265_amd/csrc/grid_resize_host.h \
                   p265_amd/csrc/grid_host.h p265_amd/csrc/resize_host.h p265_amd/csrc/resize_math.h \
                   p265_amd/csrc/export_host.h include/p265r.h
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=all \
		-o $(GRID_RESIZE_CHECK) tools/grid_resize_check.cpp p265_amd/csrc/grid_resize_host.cpp \
		p265_amd/csrc/grid_host.cpp p265_amd/csrc/resize_host.cpp p265_amd/csrc/export_host.cpp
	$(GRID_RESIZE_CHECK)
.PHONY: grid-resize-check

# host check of job prep's short cuts (intra_prep.h prep_avail_clear, prep_filter_min_lg) against the generic
# arithmetic, exhaustive: a stand-alone CPU program (hipcc, run without a GPU), not part of `all`
PREP_CHECK ?= tools/prep_check
prep-check: tools/prep_check.hip p265_amd/csrc/intra_prep.h p265_amd/csrc/intra.h p265_amd/csrc/tables.h include/p265r.h
	$(HIPCC) --offload-arch=$(ARCH) -O2 -o $(PREP_CHECK) tools/prep_check.hip
	$(PREP_CHECK)
.PHONY: prep-check

# experiment builds: make variant V=name FLAGS="-DX=1"  ->  p265_amd/libp265r_name.so
variant:
	$(HIPCC) $(HIPFLAGS) $(FLAGS) -o p265_amd/libp265r_$(V).so $(SRC)
.PHONY: variant
