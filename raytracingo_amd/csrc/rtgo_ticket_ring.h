// rtgo_ticket_ring.h -- the arithmetic of rtgo_update_prims_device_async's tickets, free of HIP so that a stand-alone
// program can check it (tests/test_ticket_ring.py): tickets count up from 1 (0 is the ticket of an update of nothing), ticket t lives in
// slot t % kSlots until ticket t + kSlots takes it, and the context answers for the last kSlots tickets it issued.
#pragma once

#include <cstdint>

namespace rtgo {

struct TicketRing {
    static constexpr uint64_t kSlots = 64;
    uint64_t next = 1;   // the next ticket
    static unsigned int slot(uint64_t ticket) { return (unsigned int)(ticket % kSlots); }
    // the ticket was issued and its slot has not been taken since
    bool holds(uint64_t ticket) const { return ticket >= 1 && ticket < next && next - ticket <= kSlots; }
    // the next ticket's slot holds an earlier ticket, whose event has to have completed before the slot is used again
    bool next_reuses_a_slot() const { return next > kSlots; }
};

}  // namespace rtgo
