/*
 * popsift/popsift.h -- PopSift / SiftJob, the asynchronous front end of the drop-in API.
 * Replaces popsift.h:40-167.  Same calls and ownership rules:
 *   - enqueue() copies the image and returns at once; the caller owns the SiftJob*
 *   - SiftJob::get() blocks and returns a Features* the caller must delete
 *   - uninit() must be called before the PopSift object goes away
 * What differs underneath: no CUDA / Boost in this header; work is spread over
 * every visible MI355X (POPSIFT_DEVICES, default "all") with several extraction
 * contexts per GPU (POPSIFT_CONTEXTS_PER_DEVICE, default 4), each with its own
 * HIP stream and buffers, behind the C ABI of popsift_hip.h.  Jobs complete through
 * their own futures, so any number of PopSift objects may coexist in a process.
 */
#pragma once

#include <condition_variable>
#include <future>
#include <mutex>
#include <queue>
#include <thread>
#include <vector>

#include <sched.h> /* cpu_set_t: a worker's CPUs */

#include "features.h"
#include "sift_conf.h"
#include "sift_extremum.h"

struct popsift_hip_ctx;

namespace popsift {
/** Extension: a caller-supplied keypoint for PopSift::enqueue(w, h, img, frames), the layout of popsift_hip_frame
 *  (include/popsift_hip.h, where the octave / level rule and the validity rules are written down).  Position and sigma in
 *  input-image units, as Feature reports them; orientation in radians, used when the job does not compute orientations. */
struct Frame {
    float xpos, ypos, sigma, orientation;
    int   octave = -1; /* -1: derived from sigma */
    int   level = -1;  /* -1: derived from sigma */
};
}  // namespace popsift

class SiftJob {
    std::promise<popsift::FeaturesBase*> _p;
    std::future<popsift::FeaturesBase*>  _f;
    int            _w;
    int            _h;
    unsigned char* _imageData; /* this job's copy of the image, in a recycled block of the pinned pool (features.h) */
    unsigned char* _mask = nullptr; /* ... and of its mask (PopSift::enqueueMasked), behind the image in the same block */
    bool           _is_float;
    bool           _pinned = false;

public:
    /** byte image, values 0..255; extension: mask, w * h bytes tightly packed (non-zero = visible) or null, copied too */
    SiftJob(int w, int h, const unsigned char* imageData, const unsigned char* mask = nullptr);
    /** float image, values [0..1[ */
    SiftJob(int w, int h, const float* imageData, const unsigned char* mask = nullptr);
    ~SiftJob();

    popsift::FeaturesHost* get();  // same as getHost()
    popsift::FeaturesBase* getBase();
    popsift::FeaturesHost* getHost();
    popsift::FeaturesDev*  getDev();

    /** fulfil the promise (called by the worker) */
    void setFeatures(popsift::FeaturesBase* f);

    int                  getWidth() const { return _w; }
    int                  getHeight() const { return _h; }
    bool                 isFloat() const { return _is_float; }
    const unsigned char* getImageData() const { return _imageData; }
    /** extension: the job's image copy is page-locked (the worker then uploads it without a staging copy) */
    bool                 isPinned() const { return _pinned; }
    /** extension: the job's copy of its mask (PopSift::enqueueMasked), null for an unmasked job */
    const unsigned char* getMask() const { return _mask; }

    /** extension: a describe job (PopSift::enqueue with frames) and its frames, copied at enqueue */
    void setFrames(const std::vector<popsift::Frame>& frames, bool computeOrientation)
    {
        _frames = frames;
        _describe = true;
        _compute_ori = computeOrientation;
    }
    /** extension: the job's descriptors come back as bytes (Config::ByteDescriptors when it was enqueued) */
    void                               setDescriptorBytes(bool on) { _desc_bytes = on; }
    bool                               wantsDescriptorBytes() const { return _desc_bytes; }
    bool                               isDescribe() const { return _describe; }
    bool                               computesOrientation() const { return _compute_ori; }
    const std::vector<popsift::Frame>& getFrames() const { return _frames; }

private:
    std::vector<popsift::Frame> _frames;
    bool                        _describe = false;
    bool                        _compute_ori = true;
    bool                        _desc_bytes = false;
};

namespace popsift {
/* extension: a sysfs cpulist ("0-15,128-143") as a CPU set; returns the number of CPUs named.  Re-entrant. */
int parseCpuList(const char* list, cpu_set_t* set);
}  // namespace popsift

class PopSift {
public:
    enum ImageMode { ByteImages, FloatImages };

    PopSift(ImageMode imode = ByteImages);
    PopSift(const popsift::Config& config,
            popsift::Config::ProcessingMode mode = popsift::Config::ExtractingMode,
            ImageMode imode = ByteImages);
    ~PopSift();

    /** Supply the configuration after default construction.  Returns false once
     *  images have been processed (the pyramid geometry is then fixed). */
    bool configure(const popsift::Config& config, bool force = false);

    /** Drains the queue, joins the workers and frees all GPU contexts. */
    void uninit();

    /** byte image, values 0..255 */
    SiftJob* enqueue(int w, int h, const unsigned char* imageData);
    /** float image, values 0..1 */
    SiftJob* enqueue(int w, int h, const float* imageData);

    /** Extension (vl_sift 'frames', OpenCV SIFT::compute): descriptors of caller-supplied keypoints instead of detected
     *  ones.  job->get() holds one Feature per frame, in the caller's order; computeOrientation = false describes each
     *  valid frame once, in frame.orientation.  Invalid frames (popsift_hip.h) come back with num_ori = 0.  The frames are
     *  copied before the call returns.  With POPSIFT_BATCH > 1 a worker batches describe jobs only with describe jobs of
     *  the same size, type and orientation mode. */
    SiftJob* enqueue(int w, int h, const unsigned char* imageData, const std::vector<popsift::Frame>& frames,
                     bool computeOrientation = true);
    SiftJob* enqueue(int w, int h, const float* imageData, const std::vector<popsift::Frame>& frames,
                     bool computeOrientation = true);

    /** Extension (OpenCV detectAndCompute(image, mask, ..)): only keypoints on visible pixels are extracted; the rule is
     *  written down in popsift_hip.h (popsift_hip_submit_batch_masked).  mask: w * h bytes, tightly packed, non-zero =
     *  visible, copied before the call returns; mask == nullptr behaves like enqueue.  With POPSIFT_BATCH > 1 a worker
     *  batches masked and unmasked extraction jobs of one size and type together. */
    SiftJob* enqueueMasked(int w, int h, const unsigned char* imageData, const unsigned char* mask);
    SiftJob* enqueueMasked(int w, int h, const float* imageData, const unsigned char* mask);

    /** deprecated blocking interface */
    inline void uninit(int /*pipe*/) { uninit(); }
    inline bool init(int /*pipe*/, int w, int h)
    {
        _last_init_w = w;
        _last_init_h = h;
        return true;
    }
    inline popsift::FeaturesBase* execute(int /*pipe*/, const unsigned char* imageData)
    {
        SiftJob* j = enqueue(_last_init_w, _last_init_h, imageData);
        if (!j) return 0;
        popsift::FeaturesBase* f = j->getBase();
        delete j;
        return f;
    }

    /** number of extraction contexts (GPUs x contexts per GPU) serving this object */
    int getContextCount() const { return (int)_workers.size(); }

private:
    struct Worker {
        std::thread      thread;
        popsift_hip_ctx* ctx = nullptr;
        int              device = 0;
        struct Pod { /* pinned staging for the POD features of a download, one per image of a batch */
            void*  p = nullptr;
            size_t cap = 0;
        };
        std::vector<Pod> pods;
        int              numa_node = -1; /* of the GPU; -1 unknown */
        bool             bind = false;   /* cpus holds the node's CPUs within the process's own affinity mask */
        cpu_set_t        cpus;
    };

    void     start_workers(int w, int h);
    SiftJob* push(SiftJob* job, int w, int h);
    void worker_loop(Worker* me);

    std::vector<Worker*>    _workers;
    std::queue<SiftJob*>    _queue;
    std::mutex              _mtx;
    std::condition_variable _cv;
    bool                    _started = false;
    bool                    _stopped = false;

    popsift::Config _config;
    popsift::Config _shadow_config;
    int             _last_init_w = 0;
    int             _last_init_h = 0;
    ImageMode       _image_mode;
    popsift::Config::ProcessingMode _proc_mode = popsift::Config::ExtractingMode;
};
