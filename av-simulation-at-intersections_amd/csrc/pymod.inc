// Python's float % for b > 0, stated once for the planner, the recorder's evaluators and the plan translation unit (jsim_plan.hip)
#ifndef JSIM_PYMOD_INC
#define JSIM_PYMOD_INC
__device__ __forceinline__ double jpl_pymod(double a, double b)
{
    double r = fmod(a, b);
    if (r != 0.0 && r < 0.0) r += b;
    return r;
}
#endif
