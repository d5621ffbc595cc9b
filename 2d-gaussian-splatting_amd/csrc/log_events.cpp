// log_events.cpp — the host half of the training log (include/surfel_log.h, LOG.md): CRC-32C, TFRecord framing and the protobuf
// wire format of a block of step Events.  Plain C++, no HIP: the file also compiles on its own with -DSURFEL_LOG_STANDALONE (what the
// sanitizer test links against a small main), where a failure leaves no message behind.  Inside the library the message goes where
// surfel_last_error() finds it.  Nothing here allocates; the callers come from a writer thread that holds no interpreter lock.
#include <stdint.h>
#include <string.h>

#include "../../include/surfel_log.h"

namespace surfel {
#ifdef SURFEL_LOG_STANDALONE
inline int log_fail(int code, const char*) { return code; }
#else
int log_fail(int code, const char* what);      // train_log.hip: api_fail without its hipError_t
#endif
}  // namespace surfel

namespace {

constexpr int E_INVALID = -1, E_LIMIT = -4;      // SURFEL_E_INVALID, SURFEL_E_LIMIT of surfel_hip.h (not included: it is the HIP side's)

struct Crc32cTable {
    uint32_t t[256];
    constexpr Crc32cTable() : t() {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ 0x82F63B78u : c >> 1;
            t[i] = c;
        }
    }
};
constexpr Crc32cTable CRC;

inline uint32_t crc32c(const uint8_t* p, int64_t n) {
    uint32_t c = 0xffffffffu;
    for (int64_t i = 0; i < n; i++) c = CRC.t[(c ^ p[i]) & 255u] ^ (c >> 8);
    return ~c;
}

inline uint32_t masked(uint32_t c) { return ((c >> 15) | (c << 17)) + 0xa282ead8u; }

inline void put_u32(uint8_t* q, uint32_t v) {
    for (int k = 0; k < 4; k++) q[k] = (uint8_t)(v >> (8 * k));
}

inline void put_u64(uint8_t* q, uint64_t v) {
    for (int k = 0; k < 8; k++) q[k] = (uint8_t)(v >> (8 * k));
}

inline int put_varint(uint8_t* q, uint64_t v) {
    int k = 0;
    while (v >= 128) {
        q[k++] = (uint8_t)(v | 128);
        v >>= 7;
    }
    q[k++] = (uint8_t)v;
    return k;
}

inline int varint_len(uint64_t v) {
    int k = 1;
    while (v >= 128) {
        v >>= 7;
        k++;
    }
    return k;
}

// header and footer around a payload that already sits at rec + 12
inline int64_t close_record(uint8_t* rec, int64_t n) {
    put_u64(rec, (uint64_t)n);
    put_u32(rec + 8, masked(crc32c(rec, 8)));
    put_u32(rec + 12 + n, masked(crc32c(rec + 12, n)));
    return n + 16;
}

struct Tag {
    const char* name;
    int len;
};
// the order in which train.py:116-117 and training_report (train.py:195-198) write them
constexpr Tag TAGS[6] = {{"train_loss_patches/dist_loss", 28}, {"train_loss_patches/normal_loss", 30}, {"train_loss_patches/reg_loss", 27},
                         {"train_loss_patches/total_loss", 29}, {"iter_time", 9}, {"total_points", 12}};
// Summary body: per value 1 (field 1) + 1 (length < 128) + [1 + 1 + tag + 1 + 4]
constexpr int value_len(int k) { return 2 + TAGS[k].len + 5; }
constexpr int SUMMARY_LEN = (2 + value_len(0)) + (2 + value_len(1)) + (2 + value_len(2)) + (2 + value_len(3)) + (2 + value_len(4)) + (2 + value_len(5));
static_assert(value_len(1) < 128 && SUMMARY_LEN >= 128 && SUMMARY_LEN < 16384, "length prefixes: one byte per value, two for the summary");
constexpr int EVENT_MAX = 9 + (1 + 5) + (1 + 2 + SUMMARY_LEN);      // wall_time, step (an int32 takes at most 5 bytes), summary

struct Record {      // SURFEL_LOG_RECORD_BYTES
    int32_t iteration, points;
    float reg_loss, total_loss, ema_dist, ema_normal, raw_total;
    uint32_t seq;
};
static_assert(sizeof(Record) == SURFEL_LOG_RECORD_BYTES, "the record of surfel_log.h");

inline uint8_t* put_value(uint8_t* q, int k, float v) {
    *q++ = 0x0A;
    *q++ = (uint8_t)value_len(k);
    *q++ = 0x0A;
    *q++ = (uint8_t)TAGS[k].len;
    memcpy(q, TAGS[k].name, (size_t)TAGS[k].len);
    q += TAGS[k].len;
    *q++ = 0x15;
    uint32_t bits;
    memcpy(&bits, &v, 4);
    put_u32(q, bits);
    return q + 4;
}

}  // namespace

extern "C" {

uint32_t surfel_log_crc32c(const void* data, int64_t n) {
    if (!data || n <= 0) return 0u;
    return crc32c(static_cast<const uint8_t*>(data), n);
}

int64_t surfel_log_frame(const void* payload, int64_t n, void* out) {
    if (!out || n < 0 || (!payload && n > 0)) return surfel::log_fail(E_INVALID, "log_frame: bad arguments");
    uint8_t* rec = static_cast<uint8_t*>(out);
    if (n > 0) memcpy(rec + 12, payload, (size_t)n);
    return close_record(rec, n);
}

int64_t surfel_log_steps_capacity(int64_t n) { return n < 0 ? 0 : n * (int64_t)(EVENT_MAX + 16); }

int64_t surfel_log_encode_steps(const void* records, int64_t n, float iter_time_ms, double wall_time, void* out, int64_t out_capacity) {
    if (n < 0 || !out || (!records && n > 0)) return surfel::log_fail(E_INVALID, "log_encode_steps: bad arguments");
    uint8_t* base = static_cast<uint8_t*>(out);
    int64_t used = 0;
    for (int64_t i = 0; i < n; i++) {
        Record r;      // (the caller's block may sit at any alignment)
        memcpy(&r, static_cast<const uint8_t*>(records) + i * SURFEL_LOG_RECORD_BYTES, sizeof r);
        if (r.iteration < 0) return surfel::log_fail(E_INVALID, "log_encode_steps: a record with a negative iteration");
        const int step_len = r.iteration ? 1 + varint_len((uint64_t)r.iteration) : 0;
        const int64_t event_len = 9 + step_len + 3 + SUMMARY_LEN;
        if (used + event_len + 16 > out_capacity) return surfel::log_fail(E_LIMIT, "log_encode_steps: out holds fewer than surfel_log_steps_capacity(n) bytes");
        uint8_t* rec = base + used;
        uint8_t* q = rec + 12;
        *q++ = 0x09;
        uint64_t wbits;
        memcpy(&wbits, &wall_time, 8);
        put_u64(q, wbits);
        q += 8;
        if (r.iteration) {
            *q++ = 0x10;
            q += put_varint(q, (uint64_t)r.iteration);
        }
        *q++ = 0x2A;
        q += put_varint(q, (uint64_t)SUMMARY_LEN);
        const float v[6] = {r.ema_dist, r.ema_normal, r.reg_loss, r.total_loss, iter_time_ms, (float)r.points};
        for (int k = 0; k < 6; k++) q = put_value(q, k, v[k]);
        used += close_record(rec, event_len);
    }
    return used;
}

}  // extern "C"
