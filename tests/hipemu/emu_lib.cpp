// emu_lib.cpp — TEST INFRASTRUCTURE ONLY.  Compiles the product's host pipeline and kernel SOURCES against the SPMD
// emulator (hip_emu.h) into tests/_build/liblariat_emu.so so that the CPU test-suite can diff kernel logic against the
// oracle without a GPU.  Never loaded by the lariat_amd package.
#define LH_EMU 1
#include "../../lariat_amd/csrc/lh_host.inc"

// the emulator's book of device allocations, for the tests (hip_emu.h); the product has no such entry points
extern "C" {
long long emu_alloc_live(void) { return emu::alloc_live(); }
long long emu_alloc_calls(void) { return emu::alloc_calls(); }
long long emu_alloc_bad_frees(void) { return emu::alloc_bad_frees(); }
void emu_alloc_fail_at(long long k) { emu::alloc_fail_at(k); }
}
