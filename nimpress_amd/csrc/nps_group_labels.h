// nps_group_labels.h -- a partition of a cohort's samples into groups (nps_samplegroups, include/nps.h) as the device holds
// it, made from the caller's label bytes.  Free of HIP (plain C++: tests/native/group_labels_driver.cpp compiles it with
// g++), like nps_subset_mask.h.  Internal header.
//
//   label    one byte per sample: the sample's group 0 .. n_groups - 1, or 255 (NPS_GROUP_NONE: scored by nobody); padded
//            with 255 to the rows' padding, a multiple of 64 samples -- the four labels of a lane-of-four are one 32-bit
//            load, and a padding sample belongs to no group
//   present  one byte per block of 256 consecutive samples (the 1 KiB of float32 a wave of the tally loads at a time): bit k
//            set when a sample of group k lies in the block; padded with zero bytes to a multiple of four bytes.  A block
//            whose byte is zero is not read by the tally, a group whose bit is clear is not added to
//   size     samples per group
#pragma once
#include <cstdint>
#include <vector>

namespace nps {

constexpr int kGroupsMax = 8;
constexpr uint8_t kGroupNone = 255;

struct GroupLabels {
    uint64_t n_samples = 0;
    int n_groups = 0;
    uint64_t size[kGroupsMax] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<uint8_t> label;
    std::vector<uint8_t> present;
};

// what nps_samplegroups_create refuses, with the first offender: a sample whose label is neither a group nor 255, or -- the
// labels being good -- no sample in any group (every label 255), or the first group without a sample
enum GroupLabelError { kGroupLabelsOk = 0, kGroupLabelBad, kGroupLabelsAllNone, kGroupLabelEmpty };
struct GroupLabelCheck {
    GroupLabelError error = kGroupLabelsOk;
    uint64_t sample = 0;  // kGroupLabelBad
    int group = 0;        // kGroupLabelEmpty
};

// label: n_samples bytes; 1 <= n_groups <= kGroupsMax (the caller has checked both)
static inline GroupLabelCheck group_labels_check(const uint8_t *label, uint64_t n_samples, int n_groups) {
    GroupLabelCheck c;
    uint64_t size[kGroupsMax] = {0, 0, 0, 0, 0, 0, 0, 0}, grouped = 0;
    for (uint64_t i = 0; i < n_samples; ++i) {
        if (label[i] == kGroupNone) continue;
        if (label[i] >= n_groups) {
            c.error = kGroupLabelBad;
            c.sample = i;
            return c;
        }
        size[label[i]] += 1;
        grouped += 1;
    }
    if (grouped == 0) {
        c.error = kGroupLabelsAllNone;
        return c;
    }
    for (int k = 0; k < n_groups; ++k)
        if (size[k] == 0) {
            c.error = kGroupLabelEmpty;
            c.group = k;
            return c;
        }
    return c;
}

// labels that group_labels_check accepts
static inline GroupLabels group_labels(const uint8_t *label, uint64_t n_samples, int n_groups) {
    GroupLabels g;
    g.n_samples = n_samples;
    g.n_groups = n_groups;
    const uint64_t n_pad = (n_samples + 63) / 64 * 64, n_blocks = (n_samples + 255) / 256;
    g.label.assign(n_pad, kGroupNone);
    g.present.assign((n_blocks + 3) / 4 * 4, 0);
    for (uint64_t i = 0; i < n_samples; ++i) {
        const uint8_t l = label[i];
        g.label[i] = l;
        if (l == kGroupNone) continue;
        g.size[l] += 1;
        g.present[i >> 8] |= (uint8_t)(1u << l);
    }
    return g;
}

}  // namespace nps
