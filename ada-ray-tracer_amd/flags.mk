# The compiler, the target and the code-generation flags of every gfx950 translation unit whose arithmetic must be the product's:
# included by ./Makefile (libart_hip.so) and by tests/device_kat/Makefile (the per-function device known-answer library), so the two
# cannot drift apart.
# -ffp-contract=off + correctly rounded div/sqrt + preserved denormals are part of the numerics
# contract: host and device must evaluate the same IEEE binary32 operations.
HIPCC   ?= /opt/rocm/bin/hipcc
ARCH    ?= gfx950
FPFLAGS := -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt -fno-gpu-flush-denormals-to-zero
# -fno-slp-vectorize: -O3 pairs adjacent f32 multiplies/adds of the triangle test into v_pk_mul_f32 / v_pk_add_f32, which costs
# register shuffles (v_mov, v_pk_mov, s_nop) and issues no faster than the single ops on gfx950: +3.5 % Mrays/s without it.
NOSLP   := -fno-slp-vectorize
OPT     := -O3
