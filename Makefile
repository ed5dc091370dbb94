# Build of the MI355X (gfx950) product and of the test-side helpers.  `python -c "import __graft_entry__ as g; g.build()"`
# drives this file.  hipcc cross-compiles gfx950 without a GPU.
HIPCC   ?= /opt/rocm/bin/hipcc
CXX     ?= g++
ARCH    ?= gfx950
# -ffp-contract=off: the decode path must round exactly like the CPU oracle (no FMA contraction)
# (the cycle counters of the trellis wavefronts, AUGX_PROF=1, are a developer build: `make prof` -> augustus_amd/libaugx_prof.so,
#  loaded instead of the product library when AUGX_LIB names it; the product is built without them)
HIPFLAGS = --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -ffp-contract=off -Wno-unused-result
CXXFLAGS = -O2 -std=c++17 -fPIC -ffp-contract=off
SRC     = augustus_amd/csrc
HOSTSRC = $(SRC)/model.cc $(SRC)/capi_model.cc $(SRC)/capi_genbank.cc $(SRC)/genes.cc $(SRC)/genbank.cc $(SRC)/evaluation.cc $(SRC)/driver.cc $(SRC)/sharded.cc
DEVHDR  = $(SRC)/device/assmemo.h $(SRC)/device/dp.h $(SRC)/device/kernels.h $(SRC)/device/dense.h $(SRC)/device/layout.h $(SRC)/device/sampler.h $(SRC)/device/snipmemo.h $(SRC)/device/launch.h
HOSTHDR = $(SRC)/model.h $(SRC)/genes.h $(SRC)/genbank.h $(SRC)/evaluation.h $(SRC)/capi_internal.h include/augx.h

all: product oracle emu
product: augustus_amd/libaugx.so augustus_amd/libaugx_smallwin.so augustus_amd/bin/augustus

# The heavy kernel families are translation units of their own, one object per block size (device/launch.h), so that `make -j`
# compiles them side by side (the whole library: ~1.5 min on 8 cores instead of ~4.5) and a kernel change rebuilds one family.
OBJ     = build/obj
FAMILIES = trellis cand forward dense
KOBJS   = $(foreach f,$(FAMILIES),$(foreach b,8 4 2,$(OBJ)/k_$(f)_$(b).o))
HOSTOBJS = $(patsubst $(SRC)/%.cc,$(OBJ)/%.o,$(HOSTSRC))
PRODFLAGS =

define KRULE
$(OBJ)/k_$(1)_$(2).o: $(SRC)/device/k_$(1).hip $(DEVHDR) include/augx.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) $$(PRODFLAGS) -DAUGX_TU_BLK=$(2) -c -o $$@ $$<
endef
$(foreach f,$(FAMILIES),$(foreach b,8 4 2,$(eval $(call KRULE,$(f),$(b)))))

$(OBJ)/decoder.o: $(SRC)/device/decoder.hip $(DEVHDR) $(HOSTHDR)
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) $(PRODFLAGS) -c -o $@ $<
$(OBJ)/%.o: $(SRC)/%.cc $(HOSTHDR) $(SRC)/device/layout.h $(SRC)/device/dp.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) $(PRODFLAGS) -c -o $@ $<

augustus_amd/libaugx.so: $(HOSTOBJS) $(OBJ)/decoder.o $(KOBJS)
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $^

# TEST INFRASTRUCTURE, built with the product because it needs the product's objects and has to travel with them: the library with
# the trellis kernels built for the smallest LDS windows kernels.h admits and the dense kernels with 8 descriptors of a block in LDS
# (SMALLWIN below; tests/test_gpu_trellis.py and tests/test_gpu_dense.py load it through AUGX_LIB; nothing of the product loads or
# ships it).  It costs three more k_trellis and three more k_dense compiles per product build.  Only those six
# objects depend on the windows: decoder.o and the other families lay out nothing by them (compiled with the flags they differ from the
# product's objects in the compilation-unit id alone, which hipcc hashes from the options; with -fuse-cuid=none they are the same
# bytes), so everything else is the product's own object
SWOBJ = build/obj_smallwin
define SWRULE
$(SWOBJ)/k_$(1)_$(2).o: $(SRC)/device/k_$(1).hip $(DEVHDR) include/augx.h
	@mkdir -p $(SWOBJ)
	$(HIPCC) $(HIPFLAGS) $$(SMALLWIN) -DAUGX_TU_BLK=$(2) -c -o $$@ $$<
endef
$(foreach f,trellis dense,$(foreach b,8 4 2,$(eval $(call SWRULE,$(f),$(b)))))
augustus_amd/libaugx_smallwin.so: $(HOSTOBJS) $(OBJ)/decoder.o $(filter-out $(OBJ)/k_trellis_% $(OBJ)/k_dense_%,$(KOBJS)) $(foreach f,trellis dense,$(foreach b,8 4 2,$(SWOBJ)/k_$(f)_$(b).o))
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $^

# developer builds, objects of their own, loaded instead of the product library when AUGX_LIB names them:
#   make prof                                   cycle counters of the trellis wavefronts (AUGX_PROF=1) -> augustus_amd/libaugx_prof.so
#   make variant NAME=x FLAGS="-DAUGX_..."      any other set of build-time switches             -> augustus_amd/libaugx_x.so
prof:
	$(MAKE) variant NAME=prof FLAGS=-DAUGX_PROFILE
variant:
	$(MAKE) OBJ=build/obj_$(NAME) PRODFLAGS="$(FLAGS)" build/obj_$(NAME)/libaugx_variant.so
	cp build/obj_$(NAME)/libaugx_variant.so augustus_amd/libaugx_$(NAME).so
$(OBJ)/libaugx_variant.so: $(HOSTOBJS) $(OBJ)/decoder.o $(KOBJS)
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $^

augustus_amd/bin/augustus: $(SRC)/augustus_main.cc augustus_amd/libaugx.so
	@mkdir -p augustus_amd/bin
	$(HIPCC) -O2 -o $@ $(SRC)/augustus_main.cc -Laugustus_amd -laugx -Wl,-rpath,'$$ORIGIN/..'

# ---- test infrastructure (never linked into the product) ----
oracle: oracle/libghmm_twin.so
oracle/libghmm_twin.so: oracle/ghmm_twin.cc include/augx.h
	$(CXX) $(CXXFLAGS) -shared -o $@ oracle/ghmm_twin.cc

emu: build/libaugx_emu.so build/libaugx_emu_pl1.so build/libaugx_emu_slowq.so build/libaugx_emu_smallwin.so build/libaugx_emu_dense_seg.so
build/libaugx_emu.so: tests/emu/emu.cc $(DEVHDR) include/augx.h
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -shared -o $@ tests/emu/emu.cc
# the same emulator with one plane of transition terms in (emulated) LDS: pieces with two GC classes then take the path
# that pieces with more than eight take in the product
build/libaugx_emu_pl1.so: tests/emu/emu.cc $(DEVHDR) include/augx.h
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -DAUGX_MAXPL_LDS=1 -shared -o $@ tests/emu/emu.cc
# the same emulator with a slow-queue threshold of 5 (kernels.h: SLOWQ_AT): candTile then flushes its queue of exon candidates that
# need the general formula before it is full, and moves the rest to the front, on ordinary inputs
build/libaugx_emu_slowq.so: tests/emu/emu.cc $(DEVHDR) include/augx.h
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -DAUGX_SLOWQ_AT=5 -shared -o $@ tests/emu/emu.cc

# the same emulator with the smallest LDS windows of the trellis that kernels.h admits (its static_asserts next to ITEM_CAP): the reads
# of predecessor values back from HBM and the candidates beyond the LDS staging, rare in the product, are then the common case; and
# with 8 descriptors of a block of the dense kernels in LDS instead of 64 (dense.h: UDCAP): most are then read from HBM, which the
# product's bound of 16 descriptors per base never lets happen
SMALLWIN = -DAUGX_ITEM_CAP=1024 -DAUGX_LIST_WIN=128 -DAUGX_VIG_WIN=128 -DAUGX_UDCAP=8
build/libaugx_emu_smallwin.so: tests/emu/emu.cc $(DEVHDR) include/augx.h
	@mkdir -p build
	$(CXX) $(CXXFLAGS) $(SMALLWIN) -shared -o $@ tests/emu/emu.cc

# the emulator plus an entry that decodes the pieces of a dense model in segments (dense.h: denseTiles; tests/test_emu_dense_seg.py)
build/libaugx_emu_dense_seg.so: tests/emu/emu_dense_seg.cc tests/emu/emu.cc $(DEVHDR) include/augx.h
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -shared -o $@ tests/emu/emu_dense_seg.cc

ref:
	$(MAKE) -C oracle -j8

clean:
	rm -rf build augustus_amd/libaugx.so augustus_amd/libaugx_smallwin.so augustus_amd/bin oracle/libghmm_twin.so
.PHONY: all product prof variant oracle emu ref clean
