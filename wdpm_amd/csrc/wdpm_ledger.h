/*
 * wdpm_ledger.h — the launch ledger (include/wdpm.h: wdpm_launch_ledger).  One process-global counter per kernel instantiation
 * the library contains, counted on the host where a launch is queued, per state of the switches the host hands the kernel
 * (WDPM_LEDGER_*).  Internal; host code only: no HIP call, nothing on the device.
 *
 * The table is complete when the library is loaded: every WDPM_LEDGER / WDPM_LEDGER_T names the kernel it counts by address, and
 * the static member of WdpmLedgerSlot<kernel, template arguments...> registers that instantiation's name during the library's
 * static initialisation - whether or not it is ever launched.  A launch site without its line is missing from the table, an
 * instantiation with other arguments than it launches is named wrongly: tests/test_launch_ledger.py compares the table with the
 * kernel symbols of the built device code.  The template arguments must be written out in full (defaults included), as literals
 * of the parameter's type (true / false for a bool): the name is made from them.
 */
#ifndef WDPM_LEDGER_H
#define WDPM_LEDGER_H

#include <string>
#include <type_traits>

#include "../../include/wdpm.h"

/* wdpm_capi.hip (the ledger table): `pretty` is the __PRETTY_FUNCTION__ of wdpm_ledger_pretty<kernel> (the kernel's unqualified name is taken from
 * it), `args` the template argument list ("<0, false>" or "") */
int wdpm_ledger_register(const char *pretty, const char *args);
void wdpm_ledger_count(int slot, int switches);      /* relaxed atomics: the rank threads of a group launch concurrently */

template <auto K> inline const char *wdpm_ledger_pretty() { return __PRETTY_FUNCTION__; }

template <typename T> inline void wdpm_ledger_arg(std::string &s, T v) {
  if (!s.empty()) s += ", ";
  if constexpr (std::is_same_v<T, bool>) s += v ? "true" : "false";
  else s += std::to_string(v);
}

template <auto K, auto... A> struct WdpmLedgerSlot {
  static std::string args() {
    std::string s;
    (wdpm_ledger_arg(s, A), ...);
    return sizeof...(A) ? "<" + s + ">" : s;
  }
  static inline const int slot = wdpm_ledger_register(wdpm_ledger_pretty<K>(), args().c_str());
};

#define WDPM_LEDGER(SW, KERNEL) wdpm_ledger_count(WdpmLedgerSlot<&KERNEL>::slot, (SW))
#define WDPM_LEDGER_T(SW, KERNEL, ...) wdpm_ledger_count(WdpmLedgerSlot<&KERNEL<__VA_ARGS__>, __VA_ARGS__>::slot, (SW))

#endif /* WDPM_LEDGER_H */
