// MEASUREMENT BUILD ONLY (-DSVR_ABLATIONS; included by svr_api.hip): kernel variants / launchers that give garbage on purpose or carry
// instrumentation.  Never compiled into the product library (hip_lib.build() without SVR_BUILD_ABLATIONS).
extern "C" int svr_debug_conv_timeline(void* dst_host, int64_t bytes) {     // measurement builds only (not in the public header)
    return Entry{"svr_debug_conv_timeline"}.hip(hipMemcpyFromSymbol(dst_host, HIP_SYMBOL(g_conv_tl), (size_t)bytes));
}
extern "C" int svr_debug_conv_epilogue(void* dst_host, int64_t bytes) {
    return Entry{"svr_debug_conv_epilogue"}.hip(hipMemcpyFromSymbol(dst_host, HIP_SYMBOL(g_conv_ep), (size_t)bytes));
}
