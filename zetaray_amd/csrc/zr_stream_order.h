// Ordering buffer accesses across streams: per buffer "the last write + every stream's last read", as events.  Host-only (no HIP header): the library
// instantiates these types with a HIP backend (zr_api.hip), tests/hostexec with a backend that logs.
//
// A backend supplies
//     using Stream = ...; using Event = ...;                  (copyable handles, Stream comparable with ==)
//     static int Create(Event* e);   static void Destroy(Event e);
//     static int Record(Event e, Stream s);                   (e marks this point of s's queue)
//     static int Wait(Stream s, Event e);                     (what s enqueues from here on runs behind e)
// with 0 for success; any other value is handed back to the caller unchanged.
//
// OrderPoints holds the events of one owner (a scene, a G-buffer, a pass).  A POINT is one record on one stream; every buffer a stage marks at the same
// place of its stream shares it, so a stage costs one record however many buffers it touched.  A point nobody refers to any more is recorded again
// for the next mark: events are created while the owner's streams and buffers are first touched, none on the steady-state path, and destroyed by the
// destructor.  A wait is never issued on the stream that recorded the point (its own queue already orders that), nor for a point of a stream that the
// waiting stream is already behind a later point of.
//
// StreamOrder stands for one buffer, or for a set of buffers that change hands together.  A user brackets its launches on stream s with
// AcquireRead ... MarkRead, or AcquireWrite ... MarkWritten (a read-modify-write is a write).  Neither type is thread-safe: what host threads share is
// guarded by its owner (zr_scene::mtx).  The StreamOrders of an owner are destroyed, or Reset, before its OrderPoints.
#pragma once
#include <cstdint>
#include <memory>
#include <vector>

namespace zr {

template<typename B> class OrderPoints
{
public:
    using Stream = typename B::Stream;
    using Event = typename B::Event;
    struct Point { Event ev; Stream st; uint64_t seq; int refs; };
    OrderPoints() = default;
    OrderPoints(const OrderPoints&) = delete;
    OrderPoints& operator=(const OrderPoints&) = delete;
    ~OrderPoints() { for (auto& p : points_) B::Destroy(p->ev); }

    // this place of s's queue.  (The point is free again until something is marked at it: mark before the next Record.)
    int Record(Stream s, Point** out)
    {
        Point* p = nullptr;
        for (auto& q : points_) if (q->refs == 0 && (!p || q->st == s)) { p = q.get(); if (p->st == s) break; }      // (a free one, of this stream if there is one)
        if (!p)
        {
            Event ev; if (int r = B::Create(&ev)) return r;
            points_.emplace_back(new Point{ev, s, 0, 0}); p = points_.back().get();
        }
        if (int r = B::Record(p->ev, s)) return r;
        p->st = s; p->seq = ++seq_;      // (records on one stream are issued in the order of its queue: a larger seq is a later place)
        *out = p;
        return 0;
    }
    // s goes behind p
    int Wait(Stream s, const Point* p)
    {
        if (p->st == s) return 0;
        Behind* b = nullptr;
        for (Behind& k : behind_) if (k.waiter == s && k.of == p->st) { b = &k; break; }
        if (b && b->seq >= p->seq) return 0;
        if (int r = B::Wait(s, p->ev)) return r;
        if (b) b->seq = p->seq; else behind_.push_back({s, p->st, p->seq});
        return 0;
    }

    // no stream is behind anything any more (with every StreamOrder of the owner Reset: stream handles may be reused by then)
    void Reset() { behind_.clear(); }

private:
    struct Behind { Stream waiter, of; uint64_t seq; };      // `waiter` has waited for the point `seq` of stream `of`
    std::vector<std::unique_ptr<Point>> points_;
    std::vector<Behind> behind_;
    uint64_t seq_ = 0;
};

template<typename B> class StreamOrder
{
public:
    using Points = OrderPoints<B>;
    using Point = typename Points::Point;
    using Stream = typename B::Stream;
    StreamOrder() = default;
    StreamOrder(const StreamOrder&) = delete;
    StreamOrder& operator=(const StreamOrder&) = delete;

    // s is about to read: behind the last write, if that was on another stream
    int AcquireRead(Points& pts, Stream s) { return write_ ? pts.Wait(s, write_) : 0; }
    // s is about to write: behind every other stream's last read, and behind the last write if that was on another stream
    int AcquireWrite(Points& pts, Stream s)
    {
        for (Point* r : reads_) if (int e = pts.Wait(s, r)) return e;
        return AcquireRead(pts, s);
    }
    // s has finished reading / writing at `at`, a point of its queue (shared with whatever else the stage marks there) ...
    void MarkRead(Point* at)
    {
        at->refs++;
        for (Point*& r : reads_) if (r->st == at->st) { r->refs--; r = at; return; }
        reads_.push_back(at);
    }
    // (the stream's own earlier read lies before `at` in its queue, and whoever comes next waits for `at`: that read needs no wait of its own any more)
    void MarkWritten(Point* at)
    {
        at->refs++;
        if (write_) write_->refs--;
        write_ = at;
        for (size_t i = 0; i < reads_.size(); i++) if (reads_[i]->st == at->st) { reads_[i]->refs--; reads_.erase(reads_.begin() + i); break; }
    }
    // ... or at this place of its queue, recorded here
    int MarkRead(Points& pts, Stream s) { Point* at; if (int e = pts.Record(s, &at)) return e; MarkRead(at); return 0; }
    int MarkWritten(Points& pts, Stream s) { Point* at; if (int e = pts.Record(s, &at)) return e; MarkWritten(at); return 0; }
    // forget every access (the caller knows them finished: a device synchronize)
    void Reset() { if (write_) write_->refs--; write_ = nullptr; for (Point* r : reads_) r->refs--; reads_.clear(); }
    // the stream of the last write, if there is one
    bool LastWriter(Stream* s) const { if (write_ && s) *s = write_->st; return write_ != nullptr; }

private:
    Point* write_ = nullptr;
    std::vector<Point*> reads_;      // one per stream that has read since that stream last wrote
};

} // namespace zr
