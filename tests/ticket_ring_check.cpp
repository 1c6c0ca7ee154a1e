// A stand-alone check of csrc/rtgo_ticket_ring.h, built with -fsanitize=address,undefined and run by tests/test_ticket_ring.py: a model
// of the context's 64 slots is driven through 1000 tickets, and every ticket from 0 to far beyond the last is asked about after each.
#include "rtgo_ticket_ring.h"

#include <cstdio>
#include <vector>

int main()
{
    using rtgo::TicketRing;
    TicketRing ring;
    std::vector<uint64_t> in_slot(TicketRing::kSlots, 0);   // the ticket each slot holds; 0: none yet
    int bad = 0;
    auto expect = [&](bool ok, const char* what, uint64_t t) {
        if (!ok) {
            std::printf("ticket %llu, next %llu: %s\n", (unsigned long long)t, (unsigned long long)ring.next, what);
            ++bad;
        }
    };
    expect(!ring.holds(0) && !ring.holds(1) && !ring.next_reuses_a_slot(), "a fresh ring holds nothing", 0);
    for (int issued = 1; issued <= 1000; ++issued) {
        const uint64_t t = ring.next;
        const unsigned int s = TicketRing::slot(t);
        expect(t == (uint64_t)issued, "tickets count up from 1", t);
        expect(s < in_slot.size(), "the slot lies in the ring", t);
        expect(ring.next_reuses_a_slot() == (in_slot[s] != 0), "a slot is reused exactly when it holds a ticket", t);
        expect(in_slot[s] == 0 || in_slot[s] + TicketRing::kSlots == t, "the slot's last ticket is the one 64 before", t);
        in_slot[s] = t;
        ring.next = t + 1;
        for (uint64_t q = 0; q <= t + 70; ++q) {
            const bool there = q >= 1 && in_slot[TicketRing::slot(q)] == q;   // the model: its slot still holds it
            expect(ring.holds(q) == there, "holds() disagrees with the slots", q);
        }
    }
    for (uint64_t q : {~0ull, ~0ull - 63, 1ull << 63, 1ull << 40})
        expect(!ring.holds(q), "a ticket never issued", q);
    ring.next = ~0ull;   // the far end of the counter: no overflow in the arithmetic
    expect(ring.holds(~0ull - 1) && ring.holds(~0ull - 64) && !ring.holds(~0ull - 65) && !ring.holds(~0ull) && !ring.holds(0), "at the counter's end", ~0ull);
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
