// Drives csrc/host_ticket.hpp without a device (tests/test_host_ticket_host.py): a writer thread stands in for the kernel that ships its data and then
// releases the ticket; the stream synchronisation and the nap are callables that count their calls.
//   host_ticket_host_driver <i32|u64> <case>   ->   result=<arrived|sync_failed|never_arrived> syncs=N naps=N elapsed_us=N payload=N
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <string>
#include <thread>

#include "../privacy_preserving_sfm_amd/csrc/host_ticket.hpp"

using namespace std::chrono;

template <class T>
struct Shipment {
  long payload = 0;      // what the kernel writes before the ticket
  T slot = 0;
  void Ship(T ticket) {
    payload = 42;
    __atomic_store_n(&slot, ticket, __ATOMIC_RELEASE);
  }
};

template <class T>
static int Run(const std::string& name) {
  const T ticket = sizeof(T) == 8 ? (T)0x100000007ull : (T)7;
  Shipment<T> sh;
  int syncs = 0, naps = 0;
  bool sync_ok = true, sync_ships = false;
  auto sync = [&] { ++syncs; if (sync_ships) sh.Ship(ticket); return sync_ok; };
  auto nap = [&] { ++naps; std::this_thread::sleep_for(microseconds(50)); };
  long spin_us = 1500;
  bool sync_first = false;
  microseconds give_up = seconds(2);
  long writer_after_us = -1;
  if (name == "present") sh.Ship(ticket);
  else if (name == "writer_in_the_spin") writer_after_us = 200;
  else if (name == "writer_in_the_naps") { writer_after_us = 20000; spin_us = 100; }
  else if (name == "writer_never_nap") { writer_after_us = 20000; spin_us = -1; }
  else if (name == "give_up") { give_up = milliseconds(50); spin_us = 100; }
  else if (name == "give_up_sync_ships") { give_up = milliseconds(50); spin_us = 100; sync_ships = true; }
  else if (name == "give_up_sync_fails") { give_up = milliseconds(50); spin_us = 100; sync_ok = false; }
  else if (name == "sync_first") { give_up = milliseconds(50); spin_us = 0; sync_first = true; sync_ships = true; }
  else if (name == "sync_first_fails") { give_up = milliseconds(50); spin_us = 0; sync_first = true; sync_ok = false; }
  else { fprintf(stderr, "unknown case %s\n", name.c_str()); return 2; }
  std::thread writer;
  if (writer_after_us >= 0) writer = std::thread([&] { std::this_thread::sleep_for(microseconds(writer_after_us)); sh.Ship(ticket); });
  const auto t0 = steady_clock::now();
  const ppsfm::TicketWait w = ppsfm::WaitHostTicket(&sh.slot, ticket, spin_us, sync, sync_first, give_up, nap);
  const long long elapsed = duration_cast<microseconds>(steady_clock::now() - t0).count();
  const long payload = w == ppsfm::TicketWait::kArrived ? sh.payload : -1;      // (behind the acquire fence of an arrival)
  if (writer.joinable()) writer.join();
  printf("result=%s syncs=%d naps=%d elapsed_us=%lld payload=%ld\n",
         w == ppsfm::TicketWait::kArrived ? "arrived" : (w == ppsfm::TicketWait::kSyncFailed ? "sync_failed" : "never_arrived"), syncs, naps, elapsed, payload);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s <i32|u64> <case>\n", argv[0]); return 2; }
  const std::string type = argv[1];
  if (type == "i32") return Run<int32_t>(argv[2]);
  if (type == "u64") return Run<unsigned long long>(argv[2]);
  fprintf(stderr, "unknown ticket type %s\n", type.c_str());
  return 2;
}
