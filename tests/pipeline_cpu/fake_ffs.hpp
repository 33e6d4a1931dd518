// fake_ffs.hpp -- controls and records of fake_ffs.cc, the stand-in for the ffs_* calls host/batch_pipeline.cc makes.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "ffs_hip.h"

namespace fake {

uint32_t checksum(const uint8_t* p, size_t n);   // FNV-1a

// A context is an id and the size of a decoded frame (what ffs_submit reads per frame).  Owned by the fake until reset().
ffs_ctx* make_ctx(int id, size_t frame_bytes);
void reset();   // frees the contexts, forgets records and switches (every stream must have been destroyed)

// switches
void block_waits();              // ffs_wait blocks ...
void release_waits();            // ... until this
void fail_submit(int nth);       // the nth submit of the run (1-based) returns FFS_ERR_DEVICE
void move_buffer_after_heap_batch(bool on);   // a batch that came from outside the staging area makes it grow -- and move

struct Submit {
    int ctx = 0;
    uint32_t first = 0, n = 0;
    bool encoded = false;
    size_t buffer_bytes = 0;
    std::vector<long long> offset;   // encoded: where each chunk lay in the stream's staging area, -1: outside it (the heap)
};
std::vector<Submit> submits();
int submits_so_far();
bool submit_has_failed();
int max_in_flight(int ctx);      // most batches of the context submitted and not yet waited for
int streams_made(int ctx);
int buffer_moves();
int protocol_errors();           // a stream submitted twice without a wait, a wait without a submit, a foreign pixel pointer

}  // namespace fake
