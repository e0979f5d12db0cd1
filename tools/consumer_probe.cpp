// consumer_probe.cpp — one twhost::Consumer on the stub backend (host/stub_twflow.cpp), fed so that what it does is the
// same from run to run: every request is queued BEFORE the thread starts, so the takes are batch, batch, ... and the tail,
// and every engine call comes from the one consumer thread.  With TW_STUB_TRACE set the stub records those calls; this
// program prints the other half of the result, the responses in arrival order.  tools/consumer_trace.py builds and runs it
// (against any commit's twhost.cpp); tests/test_host_consumer_steps.py asserts on a subset of its cases.
//
//   consumer_probe <decode threads> <resident budget, bytes> <batch> <script ...>
//     R <expected> <target>                  a pair of files
//     M <w> <h> <first a> <first b>          an in-memory pair (gray, filled with 7 except for pixel 0)
//     I <x,y,w,h[;x,y,w,h ...]>              ignore rectangles of the NEXT pair (Request::ignore)
//     D <tol> <min>                          residual for the whole run (PairExtras::residual, ::residualMin); a response then
//                                            ends in " changes <count>: [x,y diff=<n> unexplained=<n> max=<diff>,<unexplained>] ..."
//     S <radius>                             shift for the whole run (PairExtras::shift); a response then ends in
//                                            " shift <x>,<y> applied=<0|1>"
//     O <dir> <tol>                          diff images for the whole run (PairExtras::overlayDir, ::overlayTol); the response
//                                            of a pair that got one then ends in " overlay <path>"
//     B <rows>                               shift bands for the whole run (PairExtras::shiftBands); a response then ends in
//                                            " bands <count>: [y,rows dy=<dy> applied=<0|1>] ..."
//     G <gap>                                hit regions for the whole run (PairExtras::regions); a response then ends in
//                                            " regions <count>: [x,y,w,h n=<hits> peak=(x,y,dx,dy)] ... of: <index per vector>"
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <string>
#include <vector>

#include "../tidal-wave_amd/host/twhost.h"

using namespace twhost;
extern "C" void tw_stub_resident_calls(long* kept, long* image_pairs, long* released);

int main(int argc, char** argv)
{
    if (argc < 4) return 2;
    const int decode_threads = atoi(argv[1]);
    const long long budget = atoll(argv[2]);
    const int batch = atoi(argv[3]);
    MessageQueue<Request> req;
    MessageQueue<Response> res;
    ConsumerShared shared;
    shared.residentBytes = budget;
    shared.stats.assign(1, ConsumerStats());
    tw_params params;
    tw_default_params(&params);
    std::vector<std::unique_ptr<std::vector<uint8_t>>> raw;
    int asked = 0;
    std::vector<Rect> ignore;
    for (int i = 4; i < argc; i++) {
        const std::string op = argv[i];
        if (op == "G" && i + 1 < argc) {
            shared.extras.regions = atoi(argv[++i]);
            continue;
        }
        if (op == "D" && i + 2 < argc) {
            shared.extras.residual = atoi(argv[++i]);
            shared.extras.residualMin = atoi(argv[++i]);
            continue;
        }
        if (op == "S" && i + 1 < argc) {
            shared.extras.shift = atoi(argv[++i]);
            continue;
        }
        if (op == "O" && i + 2 < argc) {
            shared.extras.overlayDir = argv[++i];
            shared.extras.overlayTol = atoi(argv[++i]);
            continue;
        }
        if (op == "B" && i + 1 < argc) {
            shared.extras.shiftBands = atoi(argv[++i]);
            continue;
        }
        if (op == "I" && i + 1 < argc) {
            const char* p = argv[++i];
            Rect rc;
            int used = 0;
            while (sscanf(p, "%d,%d,%d,%d%n", &rc.x, &rc.y, &rc.width, &rc.height, &used) == 4) {
                ignore.push_back(rc);
                p += used;
                if (*p == ';') p++;
            }
            continue;
        }
        Request r;
        r.threshold = 5.0;
        r.span = 10;
        r.ignore.swap(ignore);
        if (op == "R" && i + 2 < argc) {
            r.expect_image = argv[i + 1];
            r.target_image = argv[i + 2];
            i += 2;
        } else if (op == "M" && i + 4 < argc) {
            const int w = atoi(argv[i + 1]), h = atoi(argv[i + 2]);
            for (int q = 0; q < 2; q++) {
                raw.emplace_back(new std::vector<uint8_t>((size_t)w * (size_t)h, 7));
                (*raw.back())[0] = (uint8_t)atoi(argv[i + 3 + q]);
            }
            r.expect_image = "raw_expected_" + std::to_string(asked);
            r.target_image = "raw_target_" + std::to_string(asked);
            r.raw.expect = raw[raw.size() - 2]->data();
            r.raw.target = raw[raw.size() - 1]->data();
            r.raw.width = w;
            r.raw.height = h;
            r.raw.stride = w;
            i += 4;
        } else {
            fprintf(stderr, "bad script at %s\n", argv[i]);
            return 2;
        }
        req.push(std::move(r));
        asked++;
    }
    {
        Consumer c(0, req, res, params, batch, decode_threads, 1, &shared);
        c.start();
        for (int k = 0; k < asked; k++) {
            Response r;
            if (!res.tryPop(r)) return 3;
            printf("%s|%s|%s|%s|%dx%d|span %d|threshold %g|", r.status.c_str(), r.reason.c_str(), r.expect_image.c_str(),
                   r.target_image.c_str(), r.width, r.height, r.span, r.threshold);
            for (const Vector& v : r.vectors) printf(" (%d,%d,%g,%g)", v.x, v.y, v.dx, v.dy);
            if (r.hasRegions) {
                printf(" regions %d:", r.regionCount);
                for (const Region& g : r.regions)
                    printf(" [%d,%d,%d,%d n=%d peak=(%d,%d,%g,%g)]", g.x, g.y, g.width, g.height, g.count, g.peak_x, g.peak_y,
                           g.peak_dx, g.peak_dy);
                printf(" of:");
                for (int k : r.regionOf) printf(" %d", k);
            }
            if (r.hasChanges) {
                printf(" changes %zu:", r.changes.size());
                for (const Change& c : r.changes)
                    printf(" [%d,%d diff=%d unexplained=%d max=%d,%d]", c.x, c.y, c.n_diff, c.n_unexplained, c.max_diff, c.max_unexplained);
            }
            if (r.hasShift) printf(" shift %d,%d applied=%d", r.shift.x, r.shift.y, r.shift.applied ? 1 : 0);
            if (r.hasBands) {
                printf(" bands %zu:", r.bands.size());
                for (const ShiftBand& b : r.bands) printf(" [%d,%d dy=%d applied=%d]", b.y, b.rows, b.dy, b.applied ? 1 : 0);
            }
            if (!r.overlay.empty()) printf(" overlay %s", r.overlay.c_str());
            printf("\n");
        }
        req.stop();
        c.join();
    }
    long kept = 0, pairs = 0, released = 0;
    tw_stub_resident_calls(&kept, &pairs, &released);
    printf("stopped|kept %ld|image_pairs %ld|released %ld|inflight %ld|pairs %ld|batches %ld\n", kept, pairs, released,
           shared.inflight.load(), shared.stats[0].pairs, shared.stats[0].batches);
    return 0;
}
