// switches.hpp -- the kernel-variant switches and the environment knobs of libmcedm_hip.
//
// Every kernel family that replaced another keeps its predecessor behind a switch.  A switch is one enumerator and one row of the
// table below; include/mcedm_hip.h (MCEDM_VARIANT_*), lib.py (VARIANTS, set_*) and INTEGRATION.md name it again, and
// tests/test_switches_cpu.py holds them to these rows.  Three levels, first hit wins: the plan whose entry point is executing on this
// thread (mcedm_*_plan_set_variant; a field of the plan, so two plans in one process -- on two threads or two streams -- cannot flip
// each other's kernels), the process-wide mcedm_op_set_* (kernel-level calls have no plan), the environment.
#pragma once

namespace mcedm {

enum KernelVariant { KV_CONV_WINO = 0, KV_CONV_WINO1 = 1, KV_CONV_RESIDENT = 2, KV_CONV8 = 3, KV_ATTN_FUSED = 4, KV_WGRAD_WINO = 5,
                     KV_CONV1X1_REG = 6, KV_CONV_WINO_FOLD = 7, KV_CONV_WINO_UPZ = 8, KV_CONV_WINO_SPLIT = 9, KV_COUNT = 10 };

struct KernelSwitch { const char* name; const char* env; int dflt; };
// In enumerator order: binding name (mcedm_op_set_<name>, lib.set_<name>), environment variable, value when it is unset.
static constexpr KernelSwitch kKernelSwitches[] = {
  {"conv_wino", "MCEDM_WINOGRAD", 1},
  {"conv_wino1", "MCEDM_WINO1", 0},
  {"conv_resident", "MCEDM_CONV_RESIDENT", 1},
  {"conv8", "MCEDM_CONV8", 0},
  {"attn_fused", "MCEDM_ATTN_FUSED", 1},
  {"wgrad_wino", "MCEDM_WGRAD_WINO", 1},
  {"conv1x1_reg", "MCEDM_CONV1X1_REG", 1},
  {"conv_wino_fold", "MCEDM_WINO_FOLD", 1},
  {"conv_wino_upz", "MCEDM_WINO_UPZ", 1},
  {"conv_wino_split", "MCEDM_WINO_SPLIT", 1},
};
static_assert(sizeof(kKernelSwitches) / sizeof(kKernelSwitches[0]) == KV_COUNT, "one row per KernelVariant");

// value of a switch: the executing plan's if >= 0, else the process-wide one if >= 0, else the environment's -- atoi of the row's
// variable, or the row's default when it is unset; read at first use, once per process, and returned as it stands
int kernel_switch(KernelVariant which);
int kernel_switch_forced(KernelVariant which);            // the plan's or the process-wide value; -1: neither is set
void set_kernel_switch(KernelVariant which, int value);   // the process-wide value: any integer, < 0 = not set

// an environment knob that is no switch: atoi of the variable, or dflt when it is unset.  Read once per process where it is used:
//   static const int v = env_int("MCEDM_...", d);
int env_int(const char* name, int dflt);

struct KernelVariants {                                    // a plan's own choices; -1 = the process default
  int v[KV_COUNT];
  KernelVariants() { for (int& x : v) x = -1; }
};
// first statement of every extern "C" function that takes a plan (null: no plan-level choice)
class VariantScope {
 public:
  template <class PlanT> explicit VariantScope(const PlanT* plan) : prev_(enter(plan ? &plan->variants : nullptr)) {}
  ~VariantScope();
  VariantScope(const VariantScope&) = delete;
  VariantScope& operator=(const VariantScope&) = delete;
 private:
  static const KernelVariants* enter(const KernelVariants* kv);   // returns the scope it replaces
  const KernelVariants* prev_;
};

}  // namespace mcedm
