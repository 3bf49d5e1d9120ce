#!/bin/bash
# build_variants/liblcf_<name>.so with extra -D flags:  bash tools/debug/build_variant.sh name -DLCF_X=1 ...
# lcf_hip.hip -- every kernel of the engine and of the sampler -- is compiled with the flags; the other objects are the
# product build's (made here if they are missing), so that the variant is a complete library.
NAME=$1; shift
R=$(cd "$(dirname "$0")/../.." && pwd)
C=$R/lightcurve_fitting_amd/csrc
mkdir -p $R/build_variants
OTHERS=$(make -s -C $C --eval 'others: ; @echo $(filter-out lcf_hip.o,$(OBJS))' others)
make -s -C $C $OTHERS || exit 1
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -I$R/include -Wno-unused-value -ffp-contract=on -mllvm -disable-machine-licm "$@" \
  -Rpass-analysis=kernel-resource-usage -c -o $R/build_variants/lcf_hip_$NAME.o $C/lcf_hip.hip 2> $R/build_variants/$NAME.resources.txt || exit 1
(cd $C && /opt/rocm/bin/hipcc -fPIC --offload-arch=gfx950 -shared -o $R/build_variants/liblcf_$NAME.so $R/build_variants/lcf_hip_$NAME.o $OTHERS) || exit 1
grep -A12 "k_solo_runILi5ELi1ELb1ELi2ELi1ELb0E" $R/build_variants/$NAME.resources.txt | grep -E "VGPRs:|Spill|Scratch" | tr '\n' ' '; echo " <- $NAME"
