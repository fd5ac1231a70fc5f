// The layout of a driver's device state block: typed arrays in ONE allocation, in the order they are added, each starting at a
// multiple of `align` bytes from the block's base.  add() says where an array goes and which pointer shall receive its address,
// bytes() is what to allocate, bind() sets the pointers -- size, offset and pointer type of an array are stated in one place.
// A range that is copied or cleared as a whole is ONE entry; the caller sets the pointers into it after bind().
// Host code on the standard library alone (tests/hipemu/layout_selftest.cpp includes nothing else).
#pragma once
#include <cstddef>
#include <cstring>
#include <utility>
#include <vector>

namespace robo {

class BlockLayout {
public:
    explicit BlockLayout(size_t align) : align_(align) {}
    // count * sizeof(T) bytes at the returned offset; count 0 takes no space (its field gets the next array's address)
    template <class T>
    size_t add(T** field, size_t count) {
        const size_t at = bytes_;
        fields_.emplace_back(field, at);
        bytes_ += (count * sizeof(T) + align_ - 1) / align_ * align_;
        return at;
    }
    template <class T>
    size_t add(const T** field, size_t count) {
        return add(const_cast<T**>(field), count);
    }
    size_t bytes() const { return bytes_; }
    void bind(void* base) const {
        for (const auto& f : fields_) {
            char* p = static_cast<char*>(base) + f.second;
            std::memcpy(f.first, &p, sizeof(p));       // the field is a T* of any T: set as bytes, not through a void**
        }
    }

private:
    size_t align_, bytes_ = 0;
    std::vector<std::pair<void*, size_t>> fields_;      // (address of the field, offset)
};

}  // namespace robo
