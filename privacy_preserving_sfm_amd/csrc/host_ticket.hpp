// The host's wait for a ticket that a kernel releases, at system scope, into pinned host memory behind the data it ships (the LM loop's
// scalars, the conjugate-gradient state, a four-view model's errors).  A stream synchronisation wakes the caller ~10 us after the kernel has
// ended, and every microsecond of that is an idle device in the middle of an iteration - so the host polls the ticket instead:
//   - a busy spin for as long as such a look can reasonably take (spin_us), then 50 us naps between polls (a spinning thread per handle would
//     burn a host core per GPU while a large factorisation runs); spin_us < 0: never nap
//   - bounded: once give_up has passed the stream is synchronised ONCE and the ticket looked at again (a failed launch would otherwise wait
//     forever)
// Standard library only (tests/host_ticket_host_driver.cpp runs it under the sanitizers with a writer thread in the kernel's place).
#pragma once
#include <atomic>
#include <chrono>
#include <thread>

namespace ppsfm {

enum class TicketWait { kArrived, kSyncFailed, kNeverArrived };

struct TicketNap {
  void operator()() const { std::this_thread::sleep_for(std::chrono::microseconds(50)); }
};

// sync: the caller's stream synchronisation, true on success.  sync_first: synchronise before the first poll as well (what a caller that must
// never spin does: the ticket is then there).
template <class T, class Sync, class Nap = TicketNap>
TicketWait WaitHostTicket(const volatile T* slot, T ticket, long spin_us, Sync&& sync, bool sync_first = false,
                          std::chrono::microseconds give_up = std::chrono::seconds(2), Nap&& nap = Nap()) {
  if (sync_first && !sync()) return TicketWait::kSyncFailed;
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned pauses = 0; *slot != ticket; ++pauses) {
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
    __builtin_ia32_pause();
#endif
    if ((pauses & 0xFF) != 0xFF) continue;      // (the clock: every 256 pauses)
    const auto waited = std::chrono::steady_clock::now() - t0;
    if (waited > give_up) {
      if (!sync()) return TicketWait::kSyncFailed;
      if (*slot != ticket) return TicketWait::kNeverArrived;
      break;
    }
    if (spin_us >= 0 && waited > std::chrono::microseconds(spin_us)) nap();
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  return TicketWait::kArrived;
}

}  // namespace ppsfm
