// resident_cache.h — a consumer's cache of resident expected images (Parameter::residentMB / TW_RESIDENT_MB): the expected
// image of a pair stays on the device under its file's identity, and a later pair that names the same file skips read,
// decode, arena copy and upload of it (tw_submit_image_*).  Header only, and above the C ABI alone: a small program can
// include it without twhost.cpp (tests/test_host_consumer_steps.py does).  Used from the consumer's own thread only.
#pragma once
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>

#include <algorithm>
#include <list>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/twflow.h"

namespace twhost {

// dev:ino:size:mtime(ns) of a file — what tells a rewritten baseline from the cached one ("" : no such file)
inline std::string file_identity(const std::string& path)
{
    struct stat st;
    if (stat(path.c_str(), &st) != 0) return std::string();
    char buf[160];
    snprintf(buf, sizeof(buf), "%llx:%llx:%lld:%lld.%09ld", (unsigned long long)st.st_dev, (unsigned long long)st.st_ino,
             (long long)st.st_size, (long long)st.st_mtim.tv_sec, (long)st.st_mtim.tv_nsec);
    return buf;
}

// An LRU by bytes under a budget, keyed by file identity.
//
// Invariants:
//  * An entry larger than the budget is released at once (insert never keeps it, and evicts nothing for it).
//  * Eviction never waits: it only releases the handle — the engine returns the block once no batch reads it.
//  * A pair that looked an entry up holds a pin until it is submitted.  A pinned entry that is evicted (budget, rewritten
//    or deleted file, shutdown) becomes a zombie: out of the cache, its handle alive; the first sweep() after its last
//    unpin() releases it.
//  * The image of a pair that has not answered yet is pending: one Keep, shared by the pair that kept it (the leader) and
//    the pairs behind it that name the same file (followers).  settle() ends that: into the cache on TW_OK, released
//    otherwise.
//  * Handles kept equal handles released when the cache is destroyed (every kept image is settled or registered, and
//    release_all() — the destructor — releases what is registered).
class ResidentCache {
public:
    // One resident expected image
    struct Entry {
        std::string key;
        std::vector<std::string> paths;  // every path it was asked for under (hard links share an entry)
        tw_image* img = nullptr;
        int w = 0, h = 0;
        size_t bytes = 0;
        int pins = 0;  // pairs that looked it up and are not submitted yet
        std::list<Entry*>::iterator lru;
    };
    // The image a pair's expected file becomes while that pair has not answered
    struct Keep {
        tw_image* img = nullptr;
        int w = 0, h = 0;
        bool expect_bad = false;  // the pair that kept it answered "Can't open <expected>": its content is undefined
    };

    ResidentCache(tw_engine* eng, size_t budget) : eng_(eng), budget_(eng ? budget : 0) {}
    ~ResidentCache() { release_all(); }
    ResidentCache(const ResidentCache&) = delete;
    ResidentCache& operator=(const ResidentCache&) = delete;

    bool on() const { return budget_ > 0; }
    size_t bytes() const { return bytes_; }

    // `path` has identity `key` now ("" : gone).  Seen before under another one: rewritten (or deleted) — the old image goes
    void note_identity(const std::string& path, const std::string& key)
    {
        auto seen = path_key_.find(path);
        if (seen == path_key_.end() || seen->second == key) return;
        auto old = cache_.find(seen->second);
        if (old != cache_.end()) evict(old->second.get());
        path_key_.erase(path);
    }
    // The entry of an identity, used last from now on and known under `path` too; pinned.  nullptr: not cached
    Entry* lookup(const std::string& key, const std::string& path)
    {
        Entry* en = touch(key, path);
        if (en) en->pins++;
        return en;
    }
    // The same for a pair that is being submitted this moment: no pin (nothing evicts between this and the submit)
    tw_image* image_now(const std::string& key, const std::string& path)
    {
        Entry* en = touch(key, path);
        return en ? en->img : nullptr;
    }
    bool has(const std::string& key) const { return cache_.count(key) != 0; }
    // The pending image of an identity (nullptr: none) ...
    std::shared_ptr<Keep> find_pending(const std::string& key) const
    {
        auto pk = pending_.find(key);
        return pk == pending_.end() ? nullptr : pk->second;
    }
    // ... which a pair opens when it has kept `img` (w x h) of its submitted ticket
    void open_pending(const std::string& key, const std::shared_ptr<Keep>& keep, tw_image* img, int w, int h)
    {
        keep->img = img;
        keep->w = w;
        keep->h = h;
        pending_[key] = keep;
    }
    // The pair that kept `img` has answered `r`: into the cache when it answered OK, released otherwise (a palette index
    // without an entry leaves it undefined — the pairs that read it meanwhile answer as this one does: expect_bad).  The
    // pending entry is removed only if it is still this pair's.
    void settle(const std::string& key, const std::string& path, const std::shared_ptr<Keep>& keep, tw_image* img, int w, int h,
                tw_status r)
    {
        keep->expect_bad = r == TW_E_BAD_IMAGE_FORMAT && strstr(tw_last_error(eng_), "target") == nullptr;
        keep->img = nullptr;
        auto pk = pending_.find(key);
        if (pk != pending_.end() && pk->second == keep) pending_.erase(pk);
        if (r == TW_OK) insert(key, path, img, w, h);
        else (void)tw_image_release(eng_, img);
    }
    void unpin(Entry* en) { en->pins--; }
    // release the evicted entries that no pair holds any more
    void sweep()
    {
        for (auto it = zombies_.begin(); it != zombies_.end();)
            if ((*it)->pins == 0) {
                (void)tw_image_release(eng_, (*it)->img);
                it = zombies_.erase(it);
            } else ++it;
    }
    // Manager::stop: every resident image goes back (while the engine still exists)
    void release_all()
    {
        while (!lru_.empty()) evict(lru_.back());
        sweep();
    }

private:
    Entry* touch(const std::string& key, const std::string& path)
    {
        auto it = cache_.find(key);
        if (it == cache_.end()) return nullptr;
        Entry* en = it->second.get();
        lru_.splice(lru_.begin(), lru_, en->lru);
        if (std::find(en->paths.begin(), en->paths.end(), path) == en->paths.end()) en->paths.push_back(path);
        path_key_[path] = key;
        return en;
    }
    void evict(Entry* en)
    {
        bytes_ -= en->bytes;
        lru_.erase(en->lru);
        for (const std::string& p : en->paths) {
            auto pk = path_key_.find(p);
            if (pk != path_key_.end() && pk->second == en->key) path_key_.erase(pk);
        }
        auto it = cache_.find(en->key);
        std::unique_ptr<Entry> own = std::move(it->second);
        cache_.erase(it);
        if (own->pins > 0) zombies_.push_back(std::move(own));
        else (void)tw_image_release(eng_, own->img);
    }
    void insert(const std::string& key, const std::string& path, tw_image* img, int w, int h)
    {
        const size_t bytes = ((size_t)w * (size_t)h + 255) / 256 * 256;
        if (cache_.count(key) || bytes > budget_) {  // (a pair of another batch got there first / larger than the budget)
            (void)tw_image_release(eng_, img);
            return;
        }
        while (bytes_ + bytes > budget_ && !lru_.empty()) evict(lru_.back());
        std::unique_ptr<Entry> en(new Entry());
        en->key = key;
        en->paths.push_back(path);
        en->img = img;
        en->w = w;
        en->h = h;
        en->bytes = bytes;
        lru_.push_front(en.get());
        en->lru = lru_.begin();
        bytes_ += bytes;
        path_key_[path] = key;
        cache_[key] = std::move(en);
    }

    tw_engine* const eng_;
    const size_t budget_;
    std::map<std::string, std::unique_ptr<Entry>> cache_;    // file identity -> entry
    std::map<std::string, std::string> path_key_;            // path -> the identity it was last seen with
    std::list<Entry*> lru_;                                  // front: used last
    std::list<std::unique_ptr<Entry>> zombies_;              // evicted while a pair that looked them up was not submitted yet
    std::map<std::string, std::shared_ptr<Keep>> pending_;   // identity -> the image of a pair that has not answered
    size_t bytes_ = 0;
};

}  // namespace twhost
