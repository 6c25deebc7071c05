# Builds the reference's own cost / arms / CBCA / SGM / WTA / scan-line functions into oracle/_ref/ (ignored
# by git), inside a class declaration and behind a driver that are ours (ref_core_driver.cpp), over a
# minimal cv::Mat that is ours (ref_shim/opencv_min.h).  TEST INFRASTRUCTURE ONLY.  Nothing of the reference
# is kept in this repository: the recipe copies three files out of a reference checkout, edits two lines of
# the copies, and cuts the definitions it needs out of them by line range into two include files.
#
#   make -f ref_core.mk [SM_REFERENCE_DIR=/path/to/reference]       oracle/_ref/ref_core_driver
#   make -f ref_core.mk asan                                         oracle/_ref/ref_core_driver_asan
#
# SM_REFERENCE_DIR defaults to the "reference" directory beside this repository.
SM_REFERENCE_DIR ?= $(abspath $(CURDIR)/../../reference)
OUT  = _ref
SRC  = $(OUT)/src/core
CXX ?= g++

FILES = stereoMatching.h stereoMatching.cpp main_.cpp

# -ffp-contract=off -fno-fast-math: every float operation rounds as the scalar C++ says.
# -fpermissive -w: the sources are MSVC-era C++.  Static libstdc++/libgcc: the binary also runs where only
# libc is present.  DEBUG (stereoMatching.h:36) is NOT defined: its blocks only time stages and write
# images and tables (saveTime, saveFromVm, saveFromDisp), and never touch a volume or a map.
CXXFLAGS_REF = -std=gnu++14 -ffp-contract=off -fno-fast-math -fpermissive -w -Iref_shim -I$(OUT)/src

all: $(OUT)/ref_core_driver
asan: $(OUT)/ref_core_driver_asan

# Copy, then edit the copies (two lines):
#  - stereoMatching.h:70, the switch Do_refine, 0 -> 1: cbca_core aggregates vm[1] only with it (cpp:5592),
#    and it is a compile-time constant there; sm_params.do_refine here;
#  - stereoMatching.cpp:6214, sgm()'s path count, the literal 4 -> the driver's variable: 8 paths use the
#    reference's own direction table (cpp:6207-6208), sm_params.sgm_paths here.
# Then cut, by line range:
#  class.inc, the class body (everything between our `class StereoMatching {` and `};`):
#    h:50-83     the static selectors and switches
#    h:85-351    struct Parameters with its constructor: the defaults are the reference's own
#    h:353-2697  every one-line member DECLARATION (a line of one tab, an identifier .. `);`, with the
#                `template <..>` line in front of it where there is one); definitions are not matched
#    h:634-688   genCensusCode<T> (censusCal names it in its censusFunc == 0 branch)
#    h:867-981   genCensusCode_NC_Sur, gen_cenVM_XOR
#    h:1643-1715 cal1DCost
#    h:2200-2280 min4, updateCost<T>
#    h:2699-2737 the data members
#  members.inc, definitions outside the class:
#    main:15-19  the static strings ("censusGrad", "CBCA", "sgm", ..)
#    cpp:25-48 censusGrad   271-455 calGrad, calGrad_y, calgradvm   501-534 calgradvm_1d (grad() names it)
#    603-656 grad   807-892 censusCal   1983-2110 costScan, gen_sgm_vm, the constructor
#    2210 HammingDistance   2794-2856 genTrueHorVerArms, judgeColorDif   2958-3050 calHorVerDis (the L, L_out,
#    C_D, C_D_out, minL form)   3566-3590 gen_vm_from2vm_exp   3896-3992 gen1DCumu, gen_dispFromVm,
#    genfinalVm_cbca   5354-5392 calArms (the L, L_out form)   5548-5564 initArm
#    5585-5666 cbca_core   6204-6224 sgm   6272-6416 so   6580-6826 so_T2D, so_R2L
# censusCal, grad and censusGrad cut cleanly, so the driver calls them and not their callees.
$(SRC)/.stamp: $(addprefix $(SM_REFERENCE_DIR)/,$(FILES)) ref_core.mk
	@mkdir -p $(SRC)
	cp $(addprefix $(SM_REFERENCE_DIR)/,$(FILES)) $(SRC)/
	chmod u+w $(addprefix $(SRC)/,$(FILES))
	sed -i '70s/= 0;/= 1;/' $(SRC)/stereoMatching.h
	sed -i '6214s/= 4;/= ref_core_sgm_paths;/' $(SRC)/stereoMatching.cpp
	LC_ALL=C sed -n '50,83p;85,351p' $(SRC)/stereoMatching.h > $(SRC)/class.inc
	LC_ALL=C awk 'NR >= 353 && NR <= 2697 { \
	    if ($$0 ~ /^\ttemplate *<[^;{}]*>[ \t\r]*$$/) { t = $$0; next } \
	    if ($$0 ~ /^\t[A-Za-z_][^;{}]*\)[ \t]*;[ \t\r]*(\/\/.*)?$$/) { if (t != "") print t; print } \
	    t = "" }' $(SRC)/stereoMatching.h >> $(SRC)/class.inc
	LC_ALL=C sed -n '634,688p;867,981p;1643,1715p;2200,2280p;2699,2737p' $(SRC)/stereoMatching.h >> $(SRC)/class.inc
	LC_ALL=C sed -n '15,19p' $(SRC)/main_.cpp > $(SRC)/members.inc
	LC_ALL=C sed -n '25,48p;271,455p;501,534p;603,656p;807,892p;1983,2110p;2210p;2794,2856p;2958,3050p;3566,3590p;3896,3992p;5354,5392p;5548,5564p;5585,5666p;6204,6224p;6272,6416p;6580,6826p' \
	    $(SRC)/stereoMatching.cpp >> $(SRC)/members.inc
	@touch $@

DEPS = $(SRC)/.stamp ref_core_driver.cpp ref_shim/opencv_min.h

$(OUT)/ref_core_driver: $(DEPS)
	$(CXX) -O2 $(CXXFLAGS_REF) -static-libstdc++ -static-libgcc -o $@ ref_core_driver.cpp -lm

# The same program with its own main under AddressSanitizer and UBSan, run on its own (nothing is loaded into
# another process): every Mat is a heap block of exactly its size, so a read or write past one is reported.
$(OUT)/ref_core_driver_asan: $(DEPS)
	$(CXX) -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all $(CXXFLAGS_REF) \
	    -o $@ ref_core_driver.cpp -lm

clean:
	rm -rf $(SRC) $(OUT)/ref_core_driver $(OUT)/ref_core_driver_asan

.PHONY: all asan clean
