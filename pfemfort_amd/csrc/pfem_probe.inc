// pfem_probe.inc -- the device blocks of the one-launch probes (pfem_modal_probe_*, pfem_imp_probe_*, pfem_dyn_probe_step;
// pfem_amd_diag.h).  Included once by pfem_device.hip before pfem_dynamics.inc.  A probe runs one launch of the solve's or the
// steppers' own launch code on vectors of the caller's; what the launch may not touch is found here, after it.

namespace {

// A block of a probe on the device, an allocation of its own: `front` quiet NaNs, `len` doubles, `guard` quiet NaNs.  No launch
// may read the NaNs -- a read poisons the sums -- or write them: probe_download compares the fill's bits.
struct ProbeBlock {
    DevBuf<double> d;
    const char *name = "";
    size_t len = 0, guard = 0, front = 0;
    std::vector<double> sent;              // what went up, kept where the launch must leave the block as it was
    double *p() const { return d.p + front; }
};

// host == nullptr: an output, NaN throughout, so that an entry the launch skips shows as well.  keep: the launch takes the block
// as const, and probe_download asks for the bits that went up.  front: a multiple of 2, for the 16-byte loads of the steppers.
int probe_upload(pfem_solver *s, ProbeBlock &B, const char *name, const double *host, size_t len, size_t guard, size_t front = 0, bool keep = false)
{
    B.name = name;
    B.len = len;
    B.guard = guard;
    B.front = front;
    PFEM_TRY(B.d.alloc(front + len + guard));
    std::vector<double> h(front + len + guard, std::numeric_limits<double>::quiet_NaN());
    if (host) std::memcpy(h.data() + front, host, sizeof(double) * len);
    PFEM_HIP(hipMemcpyAsync(B.d.p, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, s->stream));
    PFEM_HIP(hipStreamSynchronize(s->stream));       // (h goes out of scope)
    if (keep && host) B.sent.assign(host, host + len);
    return PFEM_OK;
}

// the block back (out may be nullptr) and the check of its guards and, for a kept block, of its entries
int probe_download(pfem_solver *s, const ProbeBlock &B, double *out, const char *who)
{
    std::vector<double> h(B.front + B.len + B.guard);
    PFEM_HIP(hipMemcpyAsync(h.data(), B.d.p, sizeof(double) * h.size(), hipMemcpyDeviceToHost, s->stream));
    PFEM_HIP(hipStreamSynchronize(s->stream));
    const double fill = std::numeric_limits<double>::quiet_NaN();
    for (size_t i = 0; i < B.front; ++i)
        if (std::memcmp(&h[i], &fill, sizeof(double)) != 0) {
            set_last_error(std::string(who) + ": the launch wrote in front of the first row of block " + B.name + " (guard entry " + std::to_string(i) + ")");
            return PFEM_ERR_HIP;
        }
    for (size_t i = B.front + B.len; i < h.size(); ++i)
        if (std::memcmp(&h[i], &fill, sizeof(double)) != 0) {
            set_last_error(std::string(who) + ": the launch wrote behind the last row of block " + B.name + " (guard entry " +
                           std::to_string(i - B.front - B.len) + ")");
            return PFEM_ERR_HIP;
        }
    if (!B.sent.empty() && std::memcmp(h.data() + B.front, B.sent.data(), sizeof(double) * B.len) != 0) {
        set_last_error(std::string(who) + ": the launch changed block " + B.name + ", which it takes as const");
        return PFEM_ERR_HIP;
    }
    if (out) std::memcpy(out, h.data() + B.front, sizeof(double) * B.len);
    return PFEM_OK;
}

}  // namespace
