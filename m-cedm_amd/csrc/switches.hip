// switches.hip -- resolution of the kernel-variant switches (switches.hpp); the one place that reads the environment.
#include <atomic>
#include <cstdlib>

#include "switches.hpp"

namespace mcedm {

static thread_local const KernelVariants* t_variants = nullptr;
const KernelVariants* VariantScope::enter(const KernelVariants* kv) {
  const KernelVariants* prev = t_variants;
  t_variants = kv;
  return prev;
}
VariantScope::~VariantScope() { t_variants = prev_; }

struct Unset : std::atomic<int> { Unset() : std::atomic<int>(-1) {} };
static Unset g_switch[KV_COUNT];                           // mcedm_op_set_*

int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

static int switch_env(KernelVariant which) {
  static std::atomic<bool> read[KV_COUNT];
  static std::atomic<int> value[KV_COUNT];
  if (!read[which].load(std::memory_order_acquire)) {
    value[which].store(env_int(kKernelSwitches[which].env, kKernelSwitches[which].dflt), std::memory_order_relaxed);
    read[which].store(true, std::memory_order_release);
  }
  return value[which].load(std::memory_order_relaxed);
}

int kernel_switch_forced(KernelVariant which) {
  if (t_variants && t_variants->v[which] >= 0) return t_variants->v[which];
  const int g = g_switch[which].load(std::memory_order_relaxed);
  return g >= 0 ? g : -1;
}

int kernel_switch(KernelVariant which) {
  const int forced = kernel_switch_forced(which);
  return forced >= 0 ? forced : switch_env(which);
}

void set_kernel_switch(KernelVariant which, int value) { g_switch[which].store(value, std::memory_order_relaxed); }

}  // namespace mcedm
