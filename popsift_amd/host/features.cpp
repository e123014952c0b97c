/* Feature / FeaturesHost (replaces features.cu:23-122,308-334). */
#include "popsift/features.h"

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iomanip>
#include <map>
#include <mutex>
#include <unistd.h>

#include "popsift_hip.h"

namespace popsift {

namespace {

/*
 * Result buffers come from a process-wide pool of pinned host blocks: the device-to-host copy of a job then runs at
 * PCIe speed straight into the memory the caller sees.  The reference pins and unpins the freshly allocated arrays
 * around every download (cudaHostRegister, features.cu:84-109), which costs milliseconds per image.  When pinned
 * memory cannot be had (no GPU runtime), blocks are plain page-aligned allocations.
 *   - size classes grow by a quarter (a 70 MB result takes an 82 MB block, not a 128 MB power of two);
 *   - blocks are allocated and released OUTSIDE the pool lock (pinning tens of MB takes tens of milliseconds);
 *   - at most POPSIFT_PINNED_CACHE_MB (default 2 GiB) of free blocks are kept, and none once the last PopSift object
 *     of the process has been shut down (trim(), called from PopSift::uninit): a long-running host application does
 *     not keep gigabytes of unswappable memory after it is done extracting.
 */
class BlockPool {
    struct Block {
        void*  p;
        size_t cap;
        bool   pinned;
        int    node; /* NUMA node of the thread that allocated (first touched) it, -1 unknown */
    };
    typedef std::pair<int, size_t> Key; /* (node, capacity): a worker reuses blocks of its own node only */
    std::mutex                _m;
    std::multimap<Key, Block> _free;
    std::map<void*, Block>       _live;
    const size_t                 MAX_CACHED = cache_limit();
    size_t                       _cached = 0;

    static size_t cache_limit()
    {
        const char* e = getenv("POPSIFT_PINNED_CACHE_MB");
        const long  mb = e ? atol(e) : 2048;
        return (size_t)(mb < 0 ? 0 : mb) << 20;
    }
    static size_t round_up(size_t n)
    {
        size_t c = 4096;
        while (c < n) c = (c + c / 4 + 4095) & ~(size_t)4095;
        return c;
    }
    static void release(const Block& b)
    {
        if (b.pinned) popsift_hip_host_free(b.p);
        else free(b.p);
    }

public:
    void* get(size_t bytes, int node, bool* pinned = 0)
    {
        const size_t cap = round_up(bytes);
        {
            std::lock_guard<std::mutex> lk(_m);
            auto                        it = _free.lower_bound(Key(node, cap));
            if (it != _free.end() && it->first.first == node && it->first.second <= cap + cap / 2) {
                Block b = it->second;
                _free.erase(it);
                _cached -= b.cap;
                _live[b.p] = b;
                if (pinned) *pinned = b.pinned;
                return b.p;
            }
        }
        Block b{popsift_hip_host_alloc(cap), cap, true, node}; /* not under the lock: other workers keep going */
        if (!b.p) {
            b.pinned = false;
            if (posix_memalign(&b.p, (size_t)sysconf(_SC_PAGESIZE), cap) != 0) return 0;
        }
        std::lock_guard<std::mutex> lk(_m);
        _live[b.p] = b;
        if (pinned) *pinned = b.pinned;
        return b.p;
    }
    void put(void* p)
    {
        if (!p) return;
        Block b;
        {
            std::lock_guard<std::mutex> lk(_m);
            auto                        it = _live.find(p);
            if (it == _live.end()) return;
            b = it->second;
            _live.erase(it);
            if (_cached + b.cap <= MAX_CACHED) {
                _cached += b.cap;
                _free.insert(std::make_pair(Key(b.node, b.cap), b));
                return;
            }
        }
        release(b);
    }
    /* give every cached block back to the system (blocks held by live results are untouched) */
    void trim()
    {
        std::multimap<Key, Block> drop;
        {
            std::lock_guard<std::mutex> lk(_m);
            drop.swap(_free);
            _cached = 0;
        }
        for (auto& kv : drop) release(kv.second);
    }
    size_t cached_bytes()
    {
        std::lock_guard<std::mutex> lk(_m);
        return _cached;
    }
};

BlockPool& pool()
{
    static BlockPool* p = new BlockPool; /* never destroyed: results may outlive static teardown */
    return *p;
}

}  // namespace

thread_local int t_pool_node = -1;

void   setPinnedPoolNode(int node) { t_pool_node = node; }
void   releasePinnedCache() { pool().trim(); }
size_t pinnedCacheBytes() { return pool().cached_bytes(); }
void*  pinnedBlockGet(size_t bytes, bool* pinned) { return pool().get(std::max<size_t>(bytes, 1), t_pool_node, pinned); }
void   pinnedBlockPut(void* block) { pool().put(block); }

FeaturesHost::FeaturesHost() : _ext(0), _ori(0) {}

FeaturesHost::FeaturesHost(int num_ext, int num_ori) : _ext(0), _ori(0) { reset(num_ext, num_ori); }

FeaturesHost::~FeaturesHost()
{
    pool().put(_ext);
    pool().put(_ori);
    pool().put(_bytes);
}

void FeaturesHost::reset(int num_ext, int num_ori)
{
    pool().put(_ext);
    pool().put(_ori);
    pool().put(_bytes);
    _bytes = 0;
    _desc_idx.clear();
    /* page-aligned like the reference (features.cu:63,72); zero-sized results stay valid objects */
    _ext = (Feature*)pool().get(std::max<size_t>((size_t)num_ext * sizeof(Feature), 1), t_pool_node);
    if (_ext == 0) {
        std::cerr << __FILE__ << ":" << __LINE__ << " Runtime error:" << std::endl
                  << "    Failed to (re)allocate memory for downloading " << num_ext << " features" << std::endl;
        exit(-1);
    }
    _ori = (Descriptor*)pool().get(std::max<size_t>((size_t)num_ori * sizeof(Descriptor), 1), t_pool_node);
    if (_ori == 0) {
        std::cerr << __FILE__ << ":" << __LINE__ << " Runtime error:" << std::endl
                  << "    Failed to (re)allocate memory for downloading " << num_ori << " descriptors" << std::endl;
        exit(-1);
    }
    setFeatureCount(num_ext);
    setDescriptorCount(num_ori);
}

void FeaturesHost::resetBytes(int num_ext, int num_ori)
{
    pool().put(_ext);
    pool().put(_ori);
    pool().put(_bytes);
    _ori = 0;
    _ext = (Feature*)pool().get(std::max<size_t>((size_t)num_ext * sizeof(Feature), 1), t_pool_node);
    _bytes = (unsigned char*)pool().get(std::max<size_t>((size_t)num_ori * 128, 1), t_pool_node);
    if (_ext == 0 || _bytes == 0) {
        std::cerr << __FILE__ << ":" << __LINE__ << " Runtime error:" << std::endl
                  << "    Failed to (re)allocate memory for downloading " << num_ext << " features / " << num_ori
                  << " byte descriptors" << std::endl;
        exit(-1);
    }
    _desc_idx.assign((size_t)num_ext * ORIENTATION_MAX_COUNT, -1);
    setFeatureCount(num_ext);
    setDescriptorCount(num_ori);
}

const unsigned char* FeaturesHost::descriptorBytes(int feature, int ori) const
{
    if (!_bytes || feature < 0 || feature >= size() || ori < 0 || ori >= _ext[feature].num_ori) return 0;
    const int idx = _desc_idx[(size_t)feature * ORIENTATION_MAX_COUNT + ori];
    return idx >= 0 ? _bytes + (size_t)idx * 128 : 0;
}

void FeaturesHost::print(std::ostream& ostr, bool write_as_uchar) const
{
    if (!_bytes) {
        for (int i = 0; i < size(); i++) _ext[i].print(ostr, write_as_uchar);
        return;
    }
    /* Feature::print's layout; the bytes are the rounded values write_as_uchar prints, saturated to 0 .. 255 */
    for (int i = 0; i < size(); i++) {
        const Feature& f = _ext[i];
        const float    sigval = 1.0f / (f.sigma * f.sigma);
        for (int ori = 0; ori < f.num_ori; ori++) {
            const unsigned char* b = descriptorBytes(i, ori);
            if (!b) continue;
            ostr << f.xpos << " " << f.ypos << " " << sigval << " 0 " << sigval << " ";
            for (int k = 0; k < 128; k++) ostr << (int)b[k] << " ";
            ostr << std::endl;
        }
    }
}

std::ostream& operator<<(std::ostream& ostr, const FeaturesHost& feature)
{
    feature.print(ostr, false);
    return ostr;
}

/* text format of features.cu:308-328 */
void Feature::print(std::ostream& ostr, bool write_as_uchar) const
{
    const float sigval = 1.0f / (sigma * sigma);
    for (int ori = 0; ori < num_ori; ori++) {
        ostr << xpos << " " << ypos << " " << sigval << " 0 " << sigval << " ";
        if (write_as_uchar) {
            for (int i = 0; i < 128; i++) ostr << roundf(desc[ori]->features[i]) << " ";
        } else {
            ostr << std::setprecision(3);
            for (int i = 0; i < 128; i++) ostr << desc[ori]->features[i] << " ";
            ostr << std::setprecision(6);
        }
        ostr << std::endl;
    }
}

std::ostream& operator<<(std::ostream& ostr, const Feature& feature)
{
    feature.print(ostr, false);
    return ostr;
}

/* ------------------------------------------------------------------------ FeaturesDev */

namespace {
[[noreturn]] void dev_fatal(const char* what, int rc)
{
    std::cerr << __FILE__ << std::endl << "E    " << what << ": " << popsift_hip_strerror(rc) << std::endl;
    exit(-1);
}
}  // namespace

FeaturesDev::FeaturesDev() : _set(0) {}

FeaturesDev::FeaturesDev(int num_ext, int num_ori) : _set(0) { reset(num_ext, num_ori); }

FeaturesDev::FeaturesDev(popsift_hip_devfeatures* adopt) : _set(adopt)
{
    int nf = 0, nd = 0;
    if (_set) popsift_hip_devfeatures_info(_set, 0, &nf, &nd);
    setFeatureCount(nf);
    setDescriptorCount(nd);
}

FeaturesDev::~FeaturesDev() { popsift_hip_devfeatures_free(_set); }

/* features.cu:148-160 */
void FeaturesDev::reset(int num_ext, int num_ori)
{
    int dev = 0;
    if (_set) popsift_hip_devfeatures_info(_set, &dev, 0, 0);
    popsift_hip_devfeatures_free(_set);
    _set = 0;
    const int rc = popsift_hip_devfeatures_alloc(dev, num_ext, num_ori, &_set);
    if (rc != POPSIFT_HIP_OK) dev_fatal("cannot allocate device feature arrays", rc);
    setFeatureCount(num_ext);
    setDescriptorCount(num_ori);
}

Feature* FeaturesDev::getFeatures()
{
    void* p = 0;
    if (_set) popsift_hip_devfeatures_ptrs(_set, &p, 0, 0);
    return (Feature*)p;
}
Descriptor* FeaturesDev::getDescriptors()
{
    void* p = 0;
    if (_set) popsift_hip_devfeatures_ptrs(_set, 0, &p, 0);
    return (Descriptor*)p;
}
int* FeaturesDev::getReverseMap()
{
    void* p = 0;
    if (_set) popsift_hip_devfeatures_ptrs(_set, 0, 0, &p);
    return (int*)p;
}
int FeaturesDev::getDevice() const
{
    int dev = 0;
    if (_set) popsift_hip_devfeatures_info(_set, &dev, 0, 0);
    return dev;
}

namespace {

/* matchAndGet / matchPairs of both set kinds: `match` and `pairs` are the C calls of the kind */
template <class Set, class Fn>
std::vector<FeaturesDev::Match> match_and_get(const Set* l, const Set* r, int l_len, Fn match)
{
    std::vector<FeaturesDev::Match> res;
    if (!l || !r) return res;
    std::vector<popsift_hip_match> raw((size_t)l_len);
    const int                      rc = match(l, r, raw.data());
    if (rc != POPSIFT_HIP_OK) dev_fatal("matching failed", rc);
    res.resize((size_t)l_len);
    for (int i = 0; i < l_len; i++) {
        const popsift_hip_match& m = raw[(size_t)i];
        res[(size_t)i] = FeaturesDev::Match{m.best, m.second, m.accept != 0, m.dist_best, m.dist_second};
    }
    return res;
}

template <class Set, class Fn>
std::vector<FeaturesDev::Pair> match_pairs(const Set* l, const Set* r, int l_len, const FeaturesDev::MatchOptions& opts, Fn pairs)
{
    static_assert(sizeof(FeaturesDev::Pair) == sizeof(popsift_hip_pair), "Pair is popsift_hip_pair");
    std::vector<FeaturesDev::Pair> res;
    if (!l || !r) return res;
    res.resize((size_t)l_len); /* always enough */
    popsift_hip_match_opts o;
    popsift_hip_default_match_opts(&o);
    o.ratio = opts.ratio;
    o.max_dist2 = opts.maxDist2;
    o.cross_check = opts.crossCheck ? 1 : 0;
    int       n = 0;
    const int rc = pairs(l, r, &o, (popsift_hip_pair*)res.data(), res.size(), &n);
    if (rc != POPSIFT_HIP_OK) dev_fatal("matching failed", rc);
    res.resize((size_t)n);
    return res;
}

}  // namespace

std::vector<FeaturesDev::Match> FeaturesDev::matchAndGet(FeaturesDev* other)
{
    return match_and_get(_set, other ? other->_set : 0, getDescriptorCount(), popsift_hip_match_sets);
}

std::vector<FeaturesDev::Pair> FeaturesDev::matchPairs(FeaturesDev* other, const MatchOptions& opts)
{
    return match_pairs(_set, other ? other->_set : 0, getDescriptorCount(), opts, popsift_hip_match_pairs);
}

namespace {
popsift_hip_guided_opts guided_opts(const FeaturesDev::GuidedOptions& opts)
{
    popsift_hip_guided_opts o;
    popsift_hip_default_guided_opts(&o);
    o.model = opts.model == FeaturesDev::GuidedOptions::Epipolar ? POPSIFT_HIP_GUIDE_EPIPOLAR : POPSIFT_HIP_GUIDE_HOMOGRAPHY;
    for (int i = 0; i < 9; i++) o.M[i] = opts.M[i];
    o.max_err = opts.maxErr;
    o.ratio = opts.ratio;
    o.max_dist2 = opts.maxDist2;
    o.cross_check = opts.crossCheck ? 1 : 0;
    return o;
}
}  // namespace

std::vector<FeaturesDev::Pair> FeaturesDev::matchGuided(FeaturesDev* other, const GuidedOptions& opts)
{
    static_assert(sizeof(Pair) == sizeof(popsift_hip_pair), "Pair is popsift_hip_pair");
    std::vector<Pair> res;
    if (!_set || !other || !other->_set) return res;
    res.resize((size_t)getDescriptorCount()); /* always enough */
    const popsift_hip_guided_opts o = guided_opts(opts);
    int                           n = 0;
    const int rc = popsift_hip_match_pairs_guided(_set, other->_set, &o, (popsift_hip_pair*)res.data(), res.size(), &n);
    if (rc != POPSIFT_HIP_OK) dev_fatal("guided matching failed", rc);
    res.resize((size_t)n);
    return res;
}

std::vector<FeaturesDev::Match> FeaturesDev::matchGuidedRows(FeaturesDev* other, const GuidedOptions& opts)
{
    if (getDescriptorCount() == 0) return std::vector<Match>(); /* the C call wants a buffer even then */
    const popsift_hip_guided_opts o = guided_opts(opts);
    return match_and_get(_set, other ? other->_set : 0, getDescriptorCount(),
                         [&o](const popsift_hip_devfeatures* l, const popsift_hip_devfeatures* r, popsift_hip_match* out) {
                             return popsift_hip_match_guided(l, r, &o, out);
                         });
}

FeaturesDev* FeaturesDev::fromHostPoints(const float* desc, const float* xy, int num, int device)
{
    popsift_hip_devfeatures* set = 0;
    const int                rc = popsift_hip_devfeatures_from_host_points(device, desc, xy, num, &set);
    if (rc != POPSIFT_HIP_OK) dev_fatal("cannot make the set from host points", rc);
    return new FeaturesDev(set);
}

std::vector<float> FeaturesDev::pairPoints(FeaturesDev* other, const std::vector<Pair>& pairs)
{
    static_assert(sizeof(Pair) == sizeof(popsift_hip_pair), "Pair is popsift_hip_pair");
    std::vector<float> pts(4 * pairs.size());
    if (pairs.empty()) return pts;
    const int rc = popsift_hip_pair_points(_set, other ? other->_set : 0, (const popsift_hip_pair*)pairs.data(), (int)pairs.size(),
                                           pts.data());
    if (rc != POPSIFT_HIP_OK) dev_fatal("cannot gather the pairs' points", rc);
    return pts;
}

FeaturesDevBytes* FeaturesDev::toBytes() const
{
    if (!_set) return 0;
    popsift_hip_bytefeatures* b = 0;
    const int                 rc = popsift_hip_bytefeatures_from_set(_set, &b);
    if (rc != POPSIFT_HIP_OK) dev_fatal("cannot make the byte set", rc);
    return new FeaturesDevBytes(b);
}

/* ------------------------------------------------------------------------ FeaturesDevBytes */

FeaturesDevBytes::FeaturesDevBytes(const unsigned char* desc, int num_ori, int device) : _set(0)
{
    const int rc = popsift_hip_bytefeatures_from_host(device, desc, num_ori, &_set);
    if (rc != POPSIFT_HIP_OK) dev_fatal("cannot allocate the byte set", rc);
}

FeaturesDevBytes::~FeaturesDevBytes() { popsift_hip_bytefeatures_free(_set); }

int FeaturesDevBytes::getDescriptorCount() const
{
    int n = 0;
    if (_set) popsift_hip_bytefeatures_info(_set, 0, &n);
    return n;
}

int FeaturesDevBytes::getDevice() const
{
    int dev = 0;
    if (_set) popsift_hip_bytefeatures_info(_set, &dev, 0);
    return dev;
}

std::vector<FeaturesDevBytes::Match> FeaturesDevBytes::matchAndGet(FeaturesDevBytes* other)
{
    return match_and_get(_set, other ? other->_set : 0, getDescriptorCount(), popsift_hip_match_bytes);
}

std::vector<FeaturesDevBytes::Pair> FeaturesDevBytes::matchPairs(FeaturesDevBytes* other, const MatchOptions& opts)
{
    return match_pairs(_set, other ? other->_set : 0, getDescriptorCount(), opts, popsift_hip_match_pairs_bytes);
}

/* ------------------------------------------------------------------------ Gallery */

Gallery::Gallery(int device) : _gallery(0)
{
    const int rc = popsift_hip_gallery_create(device, &_gallery);
    if (rc != POPSIFT_HIP_OK) dev_fatal("cannot create the gallery", rc);
}

Gallery::~Gallery() { popsift_hip_gallery_free(_gallery); }

int Gallery::add(FeaturesDevBytes* member)
{
    int       m = -1;
    const int rc = popsift_hip_gallery_add(_gallery, member ? member->getHandle() : 0, &m);
    if (rc != POPSIFT_HIP_OK) dev_fatal("cannot add to the gallery", rc);
    return m;
}

int Gallery::add(FeaturesDev* member)
{
    int       m = -1;
    const int rc = popsift_hip_gallery_add_set(_gallery, member ? member->getHandle() : 0, &m);
    if (rc != POPSIFT_HIP_OK) dev_fatal("cannot add the set to the gallery", rc);
    return m;
}

std::vector<float> Gallery::pairPoints(FeaturesDev* query, const std::vector<std::vector<Pair>>& pairs, std::vector<int>& offsets)
{
    static_assert(sizeof(Pair) == sizeof(popsift_hip_pair) && sizeof(int) == sizeof(int32_t), "Pair is popsift_hip_pair");
    if ((int)pairs.size() != size()) dev_fatal("one pair list per member", POPSIFT_HIP_ERR_INVALID);
    offsets.assign(pairs.size() + 1, 0);
    std::vector<Pair> flat;
    for (size_t m = 0; m < pairs.size(); m++) {
        flat.insert(flat.end(), pairs[m].begin(), pairs[m].end());
        offsets[m + 1] = (int)flat.size();
    }
    std::vector<float> pts(4 * flat.size());
    const int rc = popsift_hip_gallery_pair_points(query ? query->getHandle() : 0, _gallery, flat.empty() ? 0 : (const popsift_hip_pair*)flat.data(),
                                                   offsets.data(), flat.empty() ? 0 : pts.data());
    if (rc != POPSIFT_HIP_OK) dev_fatal("cannot gather the gallery's points", rc);
    return pts;
}

int Gallery::size() const
{
    int n = 0;
    popsift_hip_gallery_info(_gallery, 0, &n, 0);
    return n;
}

namespace {
/* offsets (size() + 1) and, with room, the pairs of popsift_hip_match_pairs_gallery */
std::vector<int32_t> gallery_pairs(popsift_hip_gallery* g, FeaturesDevBytes* query, const FeaturesDev::MatchOptions& opts,
                                   int n_members, std::vector<FeaturesDev::Pair>* flat)
{
    static_assert(sizeof(FeaturesDev::Pair) == sizeof(popsift_hip_pair), "Pair is popsift_hip_pair");
    std::vector<int32_t> offsets((size_t)n_members + 1, 0);
    if (!query) return offsets;
    popsift_hip_match_opts o;
    popsift_hip_default_match_opts(&o);
    o.ratio = opts.ratio;
    o.max_dist2 = opts.maxDist2;
    o.cross_check = opts.crossCheck ? 1 : 0;
    if (flat) flat->resize((size_t)n_members * (size_t)query->getDescriptorCount()); /* always enough */
    int       n = 0;
    const int rc = popsift_hip_match_pairs_gallery(query->getHandle(), g, &o, flat && !flat->empty() ? (popsift_hip_pair*)flat->data() : 0,
                                                   flat ? flat->size() : 0, offsets.data(), &n);
    if (rc != POPSIFT_HIP_OK && !(rc == POPSIFT_HIP_ERR_TOO_SMALL && !flat)) dev_fatal("matching failed", rc);
    return offsets;
}
}  // namespace

std::vector<std::vector<Gallery::Pair>> Gallery::matchPairs(FeaturesDevBytes* query, const MatchOptions& opts)
{
    const int                      n = size();
    std::vector<Pair>              flat;
    const std::vector<int32_t>     offsets = gallery_pairs(_gallery, query, opts, n, &flat);
    std::vector<std::vector<Pair>> res((size_t)n);
    for (int m = 0; m < n; m++) res[(size_t)m].assign(flat.begin() + offsets[(size_t)m], flat.begin() + offsets[(size_t)m + 1]);
    return res;
}

std::vector<int> Gallery::counts(FeaturesDevBytes* query, const MatchOptions& opts)
{
    const int                  n = size();
    const std::vector<int32_t> offsets = gallery_pairs(_gallery, query, opts, n, 0);
    std::vector<int>           res((size_t)n);
    for (int m = 0; m < n; m++) res[(size_t)m] = offsets[(size_t)m + 1] - offsets[(size_t)m];
    return res;
}

std::vector<Gallery::Link> Gallery::allLinks(int n)
{
    std::vector<Link> links;
    for (int a = 0; a < n; a++)
        for (int b = a + 1; b < n; b++) links.push_back(Link{a, b});
    return links;
}

std::vector<Gallery::Link> Gallery::sequentialLinks(int n, int k)
{
    std::vector<Link> links;
    for (int a = 0; a < n; a++)
        for (int b = a + 1; b < n && b <= a + k; b++) links.push_back(Link{a, b});
    return links;
}

std::vector<std::vector<Gallery::Pair>> Gallery::matchPairs(const std::vector<Link>& links, const MatchOptions& opts)
{
    static_assert(sizeof(Link) == sizeof(popsift_hip_link) && sizeof(Pair) == sizeof(popsift_hip_pair), "Link is popsift_hip_link");
    const int n_members = size();
    size_t    rows = 0; /* the links' left rows: always enough room for the pairs */
    for (const Link& l : links) {
        int count = 0;
        if (l.a < 0 || l.a >= n_members || l.b < 0 || l.b >= n_members) dev_fatal("a link names no member", POPSIFT_HIP_ERR_INVALID);
        popsift_hip_gallery_member(_gallery, l.a, 0, &count);
        rows += (size_t)count;
    }
    popsift_hip_match_opts o;
    popsift_hip_default_match_opts(&o);
    o.ratio = opts.ratio;
    o.max_dist2 = opts.maxDist2;
    o.cross_check = opts.crossCheck ? 1 : 0;
    std::vector<Pair>    flat(rows);
    std::vector<int32_t> offsets(links.size() + 1, 0);
    int                  n = 0;
    const int rc = popsift_hip_match_pairs_links(_gallery, links.empty() ? 0 : (const popsift_hip_link*)links.data(), (int)links.size(), &o,
                                                 flat.empty() ? 0 : (popsift_hip_pair*)flat.data(), flat.size(), offsets.data(), &n);
    if (rc != POPSIFT_HIP_OK) dev_fatal("matching the links failed", rc);
    std::vector<std::vector<Pair>> res(links.size());
    for (size_t e = 0; e < links.size(); e++) res[e].assign(flat.begin() + offsets[e], flat.begin() + offsets[e + 1]);
    return res;
}

std::vector<float> Gallery::pairPoints(const std::vector<Link>& links, const std::vector<std::vector<Pair>>& pairs, std::vector<int>& offsets)
{
    if (pairs.size() != links.size()) dev_fatal("one pair list per link", POPSIFT_HIP_ERR_INVALID);
    offsets.assign(pairs.size() + 1, 0);
    std::vector<Pair> flat;
    for (size_t e = 0; e < pairs.size(); e++) {
        flat.insert(flat.end(), pairs[e].begin(), pairs[e].end());
        offsets[e + 1] = (int)flat.size();
    }
    std::vector<float> pts(4 * flat.size());
    const int rc = popsift_hip_gallery_link_points(_gallery, links.empty() ? 0 : (const popsift_hip_link*)links.data(), (int)links.size(),
                                                   flat.empty() ? 0 : (const popsift_hip_pair*)flat.data(), offsets.data(),
                                                   flat.empty() ? 0 : pts.data());
    if (rc != POPSIFT_HIP_OK) dev_fatal("cannot gather the links' points", rc);
    return pts;
}

/* FeaturesDev::match + show_distance (features.cu:222-300): the reference prints from the device */
void FeaturesDev::match(FeaturesDev* other)
{
    const std::vector<Match> m = matchAndGet(other);
    const int                l_len = getDescriptorCount();
    const int                r_len = other ? other->getDescriptorCount() : 0;
    if (l_len == 0 || r_len == 0) return;
    std::vector<int> l_fem((size_t)l_len), r_fem((size_t)r_len);
    popsift_hip_devfeatures_download(_set, 0, l_fem.data());
    popsift_hip_devfeatures_download(other->_set, 0, r_fem.data());
    for (int i = 0; i < l_len; i++) {
        const Match& x = m[(size_t)i];
        printf("%s feat %4d [%4d] matches feat %4d [%4d] ( 2nd feat %4d [%4d] ) dist %.3f vs %.3f\n",
               x.accept ? "accept" : "reject", l_fem[(size_t)i], i, r_fem[(size_t)x.best], x.best,
               r_fem[(size_t)x.second], x.second, x.dist_best, x.dist_second);
    }
}

}  // namespace popsift
