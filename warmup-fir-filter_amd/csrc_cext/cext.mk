# cext.mk — the rules the extension libraries share.  A csrc_<NAME>/Makefile sets
#   NAME      the library: libfir_$(NAME).so, capi_$(NAME).hip, $(NAME).h, tests/c/$(NAME)_check.c
#   KERNEL    its kernel source, without the .hip
#   ID_MACRO  the macro that carries the source id into capi_$(NAME).hip
# and includes this file; make runs in that directory.  The library goes into ../fir_hip/ so it sits
# next to its ctypes loader.  It includes the header-only device helpers of ../csrc (fir_common.h,
# fir_dispatch.h) and the header-only host and device layers of this directory, compiles nothing from either
# and links against no other library of the project.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
INC := -I../../include -I../csrc -I../csrc_cext -I.
HIPFLAGS ?= -O3 -std=c++17 --offload-arch=$(ARCH) -fPIC -ffp-contract=off -Wall
OUTDIR := ../fir_hip
LIB := $(OUTDIR)/libfir_$(NAME).so
SRCS := $(KERNEL).hip capi_$(NAME).hip
OBJS := $(patsubst %.hip,build/%.o,$(SRCS))
# every object depends on all of them: a change to the shared layer rebuilds every library
HDRS := $(NAME).h ../csrc/fir_common.h ../csrc/fir_dispatch.h ../../include/fir_$(NAME).h ../../include/fir_hip.h \
	../csrc_cext/cext_capi.h ../csrc_cext/cext_launch.h ../csrc_cext/cext_device.h ../csrc_cext/cext.mk
# the source id embedded in the library (fir_$(NAME)_build_id); the Python loader checks it
BUILD_ID := $(shell python3 ../fir_hip/_srcid_ext.py $(NAME))

all: $(LIB)

build/%.o: %.hip $(HDRS)
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) $(INC) -c $< -o $@

# capi_$(NAME).o carries the build id: rebuilt whenever any source (or the Makefile) changes
build/capi_$(NAME).o: capi_$(NAME).hip $(SRCS) $(HDRS) Makefile
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) $(INC) -D$(ID_MACRO)='"$(BUILD_ID)"' -c $< -o $@

$(LIB): $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJS)

# kernel resource usage (VGPR / SGPR / spills / LDS / occupancy) of every instantiation:
#   make resource > ../../profiles/$(NAME)/resource_usage.txt
resource: $(KERNEL).hip $(HDRS)
	@$(HIPCC) $(HIPFLAGS) $(INC) --cuda-device-only -c $< -o /dev/null -Rpass-analysis=kernel-resource-usage 2>&1 | \
		grep -E "remark:" | sed -E 's/^[^ ]*: remark: //; s/ \[-Rpass-analysis=kernel-resource-usage\]//'

# Host AddressSanitizer check of the C ABI: the host code of both sources instrumented (device code
# untouched: GPU sanitizers are not used) into build/libfir_$(NAME)_asan.so, driven by the
# stand-alone tests/c/$(NAME)_check.c.  Runs on the CPU, with or without a GPU.
CLANG ?= /opt/rocm/lib/llvm/bin/clang
ASAN_HOST := -Xarch_host -fsanitize=address -Xarch_host -fno-omit-frame-pointer
ASAN_LIB := build/libfir_$(NAME)_asan.so
build/%_asan.o: %.hip $(SRCS) $(HDRS) Makefile
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) $(ASAN_HOST) $(INC) -D$(ID_MACRO)='"$(BUILD_ID)"' -c $< -o $@

$(ASAN_LIB): $(patsubst %.hip,build/%_asan.o,$(SRCS))
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $(ASAN_HOST) -o $@ $^

build/$(NAME)_check: ../../tests/c/$(NAME)_check.c $(ASAN_LIB)
	$(CLANG) -O1 -g -fsanitize=address -fno-gpu-sanitize -Wno-unused-command-line-argument -fno-omit-frame-pointer \
		-I../../include -DEXPECT_BUILD_ID='"$(BUILD_ID)"' $< -o $@ -L build -lfir_$(NAME)_asan -Wl,-rpath,$(CURDIR)/build

asan-check: build/$(NAME)_check
	ASAN_OPTIONS=detect_leaks=0:abort_on_error=1 ./build/$(NAME)_check

clean:
	rm -rf build $(LIB)

.PHONY: all clean resource asan-check
