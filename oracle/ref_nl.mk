# Builds the reference's own NL/ tree-filter code into oracle/_ref/ (ignored by git), with our driver
# ref_nl_driver.cpp around it.  TEST INFRASTRUCTURE ONLY.  Nothing of the reference is kept in this
# repository: the recipe copies eight files out of a reference checkout, adapts the copies with edit
# commands that name lines or generic tokens, and compiles them.
#
#   make -f ref_nl.mk [SM_REFERENCE_DIR=/path/to/reference]
#
# SM_REFERENCE_DIR defaults to the "reference" directory beside this repository.
SM_REFERENCE_DIR ?= $(abspath $(CURDIR)/../../reference)
NL   = $(SM_REFERENCE_DIR)/NL
OUT  = _ref
SRC  = $(OUT)/src
CXX ?= g++
CC  ?= gcc

FILES = qx_basic.h qx_basic.cpp qx_mst_kruskals_image.h qx_mst_kruskals_image.cpp \
        qx_tree_filter.h qx_tree_filter.cpp ctmf.h ctmf.c

# -ffp-contract=off: the filter's  w * (p - w * c) + c  must round after every operation.
# -fpermissive -w: the sources are MSVC-era C++ (string literals as char*, and the like).
# ctmf is compiled WITH assertions (no -DNDEBUG): an image size it cannot do then ends the program
# instead of hanging it.  Static libstdc++/libgcc: the binary also runs where only libc is present.
CXXFLAGS_REF = -O2 -ffp-contract=off -fno-fast-math -fpermissive -w -D'__int64=long long' \
               -Iref_shim -I$(SRC) -include ref_shim/ref_prefix.h
CFLAGS_REF   = -O2 -ffp-contract=off -fno-fast-math -w -UNDEBUG

all: $(OUT)/ref_nl_driver

# Copy, then adapt the copies:
#  - "unsigned char(expr)", a two-word functional cast g++ rejects, becomes "(unsigned char)(expr)";
#  - qx_tree_filter.cpp lines 38-60 hold two member templates that are never instantiated and name
#    members the class does not declare: deleted.
$(SRC)/.stamp: $(addprefix $(NL)/,$(FILES)) ref_nl.mk
	@mkdir -p $(SRC)
	cp $(addprefix $(NL)/,$(FILES)) $(SRC)/
	chmod u+w $(addprefix $(SRC)/,$(FILES))
	sed -i 's/unsigned char(/(unsigned char)(/g' $(SRC)/qx_basic.h $(SRC)/qx_basic.cpp
	sed -i '38,60d' $(SRC)/qx_tree_filter.cpp
	@touch $@

$(OUT)/ref_nl_driver: $(SRC)/.stamp ref_nl_driver.cpp $(wildcard ref_shim/*.h)
	$(CC) $(CFLAGS_REF) -c $(SRC)/ctmf.c -o $(OUT)/ctmf.o
	$(CXX) $(CXXFLAGS_REF) -static-libstdc++ -static-libgcc -o $@ ref_nl_driver.cpp \
	    $(SRC)/qx_basic.cpp $(SRC)/qx_mst_kruskals_image.cpp $(SRC)/qx_tree_filter.cpp $(OUT)/ctmf.o -lm

clean:
	rm -rf $(OUT)

.PHONY: all clean
