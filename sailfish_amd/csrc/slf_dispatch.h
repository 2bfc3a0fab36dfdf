// Run-time value -> template argument, for the host-side launchers (host code only).  A launcher nests one pick per
// compile-time switch of its kernel family; the innermost generic lambda opens with
//   if constexpr (<combination nobody launches>) return; else hipLaunchKernelGGL(...)
// and that condition is where "which instantiations exist" is written down: what it names is not instantiated.  A launcher
// with such a condition returns hipErrorInvalidValue unless the launch was reached, so a wrong condition is an error.
// The per-node sweep's condition is a constexpr function of a SweepVariant (slf_variant.h: per_node_variant_exists), which
// module_config() (slf_bind.h) asks as well: there the error is reported at module creation, on a CPU.
#pragma once
#include <type_traits>
#include "slf_kernels.h"
#include "slf_lattice.h"

namespace slf {

// calls f(std::integral_constant<T, V>{}) for the V of the list that equals v; false if none does
template <class T, T... Vs, class F>
inline bool pick(T v, F&& f) { return ((v == Vs ? (f(std::integral_constant<T, Vs>{}), true) : false) || ...); }
template <class F> inline bool pick_bool(bool v, F&& f) { return pick<bool, false, true>(v, f); }
template <class F> inline bool pick_prop(Prop p, F&& f) { return pick<int, PROP_AB, PROP_AA_EVEN, PROP_AA_ODD>((int)p, f); }

// precision of a module: f(float{}) or f(double{}), returns what f returns
template <class F> inline auto pick_real(const KernelSelector& sel, F&& f) { return sel.precision == 4 ? f(float{}) : f(double{}); }

// lattice x precision of a module: f(LR<L, R>{}), returns f's hipError_t.  D2Q9 and D3Q19, the lattices every kernel family
// is written for; any other id is an error here, never D3Q19 (D3Q15 and D3Q27 have their own picker, slf_lat.hip)
template <class L_, class R_> struct LR { using L = L_; using R = R_; };
template <class F> inline hipError_t pick_lr(const KernelSelector& sel, F&& f) {
  if (sel.lattice == D2Q9::id) return pick_real(sel, [&](auto r) { return f(LR<D2Q9, decltype(r)>{}); });
  if (sel.lattice == D3Q19::id) return pick_real(sel, [&](auto r) { return f(LR<D3Q19, decltype(r)>{}); });
  return hipErrorInvalidValue;
}

}  // namespace slf
