// term_table.h -- di_term_table: term strings (UTF-8) numbered in order of first
// appearance, and the writer of the reference's index files that text_index.cpp and the
// device builder's route share.  Host code only.
#pragma once

#include <cstdint>
#include <memory>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

struct di_term_table {
    std::vector<std::unique_ptr<char[]>> blocks;  // the terms' bytes (never moved)
    size_t block_left = 0;
    char *block_at = nullptr;
    std::vector<std::string_view> terms;  // by id
    std::unordered_map<std::string_view, uint32_t> ids;
};

namespace di {

// vocab.txt (one term a line, row order), inverted_index.idx (u64 start / end byte offsets
// per row) and inverted_index.dat (`dat`: toff[n_rows] records of u32 doc + u8 value) in
// out_dir -- create.py:45-51, formats src/utils/defaults.py:22-37.
void write_reference_files(const std::string &out_dir, const std::vector<std::string_view> &vocab,
                           const int64_t *toff, const unsigned char *dat);

}  // namespace di
