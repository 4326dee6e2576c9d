// cts_tcp_exchange_math.hpp — the closed forms of cts_tcp_exchange.h, written once for the host helpers
// (cts_tcp_exchange.cpp), the tick's planning (cts_tick_plan.hip) and its descriptor pass (cts_fill.hip): element m of
// a connection's buffer sequence, and the bytes each direction has sent after m buffers. No loop anywhere: a position
// past 2^33 costs what position 0 costs. All arithmetic is 64-bit and saturates where a malformed entry would make it
// wrap, so whatever an entry holds, a length is at most buffer_size.
#pragma once

#include <stdint.h>

#include "cts_tcp_exchange.h"

#if defined(__HIP__)
#define CTS_XCH_FN __host__ __device__ __forceinline__
#else
#define CTS_XCH_FN inline
#endif

namespace cts {

// The constants of an entry that the closed forms read.
struct ExchangeShape {
    uint64_t T, N;
    uint32_t B, pattern, P, Q;
};

CTS_XCH_FN ExchangeShape exchange_shape(const cts_tcp_exchange_state* e)
{
    return ExchangeShape{e->transfer_bytes, e->total_buffers, e->buffer_size, e->pattern, e->push_bytes, e->pull_bytes};
}

// An entry the closed forms can run on: no division by zero ahead.
CTS_XCH_FN bool exchange_shape_ok(const ExchangeShape& s)
{
    if (s.B == 0u || s.pattern > CTS_TCP_EXCHANGE_DUPLEX) return false;
    return s.pattern != CTS_TCP_EXCHANGE_PUSHPULL || (s.P != 0u && s.Q != 0u);
}

CTS_XCH_FN uint64_t exchange_ceil_div(uint64_t a, uint64_t b) { return a / b + (a % b != 0u ? 1u : 0u); }
CTS_XCH_FN uint64_t exchange_min(uint64_t a, uint64_t b) { return a < b ? a : b; }
CTS_XCH_FN uint64_t exchange_sub(uint64_t a, uint64_t b) { return a > b ? a - b : 0u; }

// What each direction of a Duplex connection sends: T rounded up to even, halved (no wrap at T = 2^64 - 1).
CTS_XCH_FN uint64_t exchange_half(uint64_t T) { return T / 2u + (T & 1u); }

// What direction d carries in total.
CTS_XCH_FN uint64_t exchange_direction_total(const ExchangeShape& s, uint32_t d)
{
    switch (s.pattern) {
        case CTS_TCP_EXCHANGE_PUSH: return d == 0u ? s.T : 0u;
        case CTS_TCP_EXCHANGE_PULL: return d == 1u ? s.T : 0u;
        case CTS_TCP_EXCHANGE_DUPLEX: return exchange_half(s.T);
        default: {
            const uint64_t C = (uint64_t)s.P + s.Q, full = s.T / C, rem = s.T % C;
            if (d == 0u) return full * s.P + exchange_min(rem, s.P);
            return full * s.Q + exchange_sub(rem, s.P);
        }
    }
}

// N, the length of the buffer sequence.
CTS_XCH_FN uint64_t exchange_total_buffers(const ExchangeShape& s)
{
    switch (s.pattern) {
        case CTS_TCP_EXCHANGE_PUSH:
        case CTS_TCP_EXCHANGE_PULL: return exchange_ceil_div(s.T, s.B);
        case CTS_TCP_EXCHANGE_DUPLEX: return 2u * exchange_ceil_div(exchange_half(s.T), s.B);
        default: {
            const uint64_t kp = exchange_ceil_div(s.P, s.B), kq = exchange_ceil_div(s.Q, s.B);
            const uint64_t C = (uint64_t)s.P + s.Q, full = s.T / C, rem = s.T % C;
            const uint64_t tail = rem <= s.P ? exchange_ceil_div(rem, s.B) : kp + exchange_ceil_div(rem - s.P, s.B);
            return full * (kp + kq) + tail;
        }
    }
}

// Element m < N of the sequence: its direction, its position in that direction's stream and its length. For PushPull
// the one 64-bit division is m / K.
CTS_XCH_FN void exchange_element(const ExchangeShape& s, uint64_t m, uint32_t& d, uint64_t& pos, uint32_t& len)
{
    const uint64_t B = s.B;
    switch (s.pattern) {
        case CTS_TCP_EXCHANGE_PUSH:
        case CTS_TCP_EXCHANGE_PULL:
            d = s.pattern == CTS_TCP_EXCHANGE_PULL ? 1u : 0u;
            pos = m * B;
            len = (uint32_t)exchange_min(B, exchange_sub(s.T, pos));
            return;
        case CTS_TCP_EXCHANGE_DUPLEX:
            d = (uint32_t)(m & 1u);
            pos = (m >> 1) * B;
            len = (uint32_t)exchange_min(B, exchange_sub(exchange_half(s.T), pos));
            return;
        default: {
            const uint64_t kp = ((uint64_t)s.P + B - 1u) / B, kq = ((uint64_t)s.Q + B - 1u) / B, K = kp + kq;
            const uint64_t y = m / K, r = m - y * K, C = (uint64_t)s.P + s.Q;
            const bool push = r < kp;
            const uint64_t in_seg = (push ? r : r - kp) * B;  // m_intraSegmentTransfer
            const uint64_t seg = push ? s.P : s.Q;
            const uint64_t G = y * C + (push ? 0u : s.P) + in_seg;
            d = push ? 0u : 1u;
            pos = y * seg + in_seg;
            len = (uint32_t)exchange_min(exchange_min(B, exchange_sub(seg, in_seg)), exchange_sub(s.T, G));
            return;
        }
    }
}

// The sequence one element at a time, for a walk that has to look at every buffer (the paced tick): seeded by one
// closed-form evaluation at m, then moved by additions only. For PushPull this is the reference's own machine
// (m_sending, m_intraSegmentTransfer, the remaining transfer); the lengths are exchange_element's.
struct ExchangeCursor {
    uint64_t left;   // PushPull: bytes left of T; otherwise bytes left of direction d's stream
    uint64_t other;  // Duplex: bytes left of the other direction's stream
    uint32_t d;      // the direction of the next buffer
    uint32_t intra;  // PushPull: m_intraSegmentTransfer

    CTS_XCH_FN void seed(const ExchangeShape& s, uint64_t m)
    {
        const uint64_t B = s.B;
        other = 0u;
        intra = 0u;
        switch (s.pattern) {
            case CTS_TCP_EXCHANGE_PUSH:
            case CTS_TCP_EXCHANGE_PULL:
                d = s.pattern == CTS_TCP_EXCHANGE_PULL ? 1u : 0u;
                left = exchange_sub(s.T, m * B);
                return;
            case CTS_TCP_EXCHANGE_DUPLEX:
                // after an odd m direction 0 is one buffer ahead of direction 1
                d = (uint32_t)(m & 1u);
                left = exchange_sub(exchange_half(s.T), (m >> 1) * B);
                other = d == 0u ? left : exchange_sub(left, B);
                return;
            default: {
                const uint64_t kp = ((uint64_t)s.P + B - 1u) / B, kq = ((uint64_t)s.Q + B - 1u) / B, K = kp + kq;
                const uint64_t y = m / K, r = m - y * K, C = (uint64_t)s.P + s.Q;
                const bool push = r < kp;
                const uint64_t in_seg = (push ? r : r - kp) * B;  // < the segment's size: r counts whole buffers
                d = push ? 0u : 1u;
                intra = (uint32_t)in_seg;
                left = exchange_sub(s.T, y * C + (push ? 0u : s.P) + in_seg);
                return;
            }
        }
    }
    // The length of the next buffer: min(B, bytes left[, segment - intra]).
    CTS_XCH_FN uint32_t len(const ExchangeShape& s) const
    {
        uint64_t n = exchange_min(s.B, left);
        if (s.pattern == CTS_TCP_EXCHANGE_PUSHPULL) n = exchange_min(n, (d == 0u ? s.P : s.Q) - intra);
        return (uint32_t)n;
    }
    // Past a buffer of n = len(s) bytes; true when the direction has changed.
    CTS_XCH_FN bool advance(const ExchangeShape& s, uint32_t n)
    {
        left -= n;
        if (s.pattern == CTS_TCP_EXCHANGE_DUPLEX) {
            const uint64_t mine = left;
            left = other;
            other = mine;
            d ^= 1u;
            return true;
        }
        if (s.pattern != CTS_TCP_EXCHANGE_PUSHPULL) return false;
        intra += n;
        if (intra < (d == 0u ? s.P : s.Q)) return false;
        d ^= 1u;
        intra = 0u;
        return true;
    }
};

// The bytes each direction has sent once the first m <= N buffers are out.
CTS_XCH_FN void exchange_position(const ExchangeShape& s, uint64_t m, uint64_t (&sent)[2])
{
    if (m >= s.N) {
        sent[0] = exchange_direction_total(s, 0u);
        sent[1] = exchange_direction_total(s, 1u);
        return;
    }
    // m < N: buffer m exists, so every segment before its own is whole and so is every buffer before it in its own
    const uint64_t B = s.B;
    switch (s.pattern) {
        case CTS_TCP_EXCHANGE_PUSH:
            sent[0] = m * B;
            sent[1] = 0u;
            return;
        case CTS_TCP_EXCHANGE_PULL:
            sent[0] = 0u;
            sent[1] = m * B;
            return;
        case CTS_TCP_EXCHANGE_DUPLEX:
            // (direction 0's last buffer, element N - 2, may be the short one)
            sent[0] = exchange_min(((m + 1u) >> 1) * B, exchange_half(s.T));
            sent[1] = (m >> 1) * B;
            return;
        default: {
            const uint64_t kp = ((uint64_t)s.P + B - 1u) / B, kq = ((uint64_t)s.Q + B - 1u) / B, K = kp + kq;
            const uint64_t y = m / K, r = m - y * K;
            sent[0] = y * s.P + (r < kp ? r * B : (uint64_t)s.P);
            sent[1] = y * s.Q + (r < kp ? 0u : (r - kp) * B);
            return;
        }
    }
}

}  // namespace cts
