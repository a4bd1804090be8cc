'use strict';
/* nd4hip — Node.js host side of the MI355X backend for nd4js's `nd.la` hot path.
 *
 * Same function names, argument meaning, result layout and error messages as the reference:
 *   matmul2     src/la/matmul.js:91-147        qr_decomp   src/la/qr.js:80-145
 *   matmul      src/la/matmul.js:150-236       lu_decomp   src/la/lu.js:24-81
 *   svd_decomp  src/la/svd.js:25 (= svd_dc, src/la/svd_dc.js:883-932)
 * Every float64 call goes through the N-API addon (nd4hip_napi.node -> libnd4hip.so -> HIP kernels).
 * There is NO CPU implementation in this package. Two ways to use it:
 *
 *   const la = require('nd4js_amd/js');                 // standalone: minimal NDArray, float64 only
 *   const nd = require('nd4js'); require('nd4js_amd/js').install(nd);
 *        // drop-in: nd.la.{matmul2,matmul,qr_decomp,lu_decomp,svd_decomp,svd_dc} run on the GPU for
 *        // float64 / int32(promoted) input, matmul2 / matmul also for complex128 paired with complex128,
 *        // float64 or int32 (results in the host module's Complex128Array); other dtypes (float32, object,
 *        // int32 x int32 matmul, complex input to the other functions) keep going to nd4js's own functions.
 */
const path = require('path');
let addon = null;
function native() {
  if (addon === null) {
    try { addon = require(process.env.ND4HIP_NAPI_ADDON || path.join(__dirname, 'nd4hip_napi.node')); }   // (override: the sanitizer build of the shim, tools/check_sanitize.sh)
    catch (e) { throw new Error('nd4hip: cannot load the N-API addon (' + e.message + '). Build it with `python -m nd4js_amd.build`; there is no CPU fallback.'); }
  }
  return addon;
}

/* ---- minimal NDArray (src/nd_array.js:128-158): dense, row-major, shape Int32Array ---- */
class NDArray {
  constructor(shape, data) {
    if (!(shape instanceof Int32Array)) throw new Error('Shape must be Int32Array.');
    if (shape.some(s => s < 1)) throw new Error(`Invalid shape: ${shape}.`);
    if (data.length !== shape.reduce((a, b) => a * b, 1)) throw new Error(`Shape [${shape}] does not match array length of ${data.length}.`);
    this.shape = shape; this.data = data; Object.freeze(this.shape.buffer);
  }
  get ndim() { return this.shape.length; }
  get dtype() {
    if (this.data instanceof Float64Array) return 'float64';
    if (this.data instanceof Float32Array) return 'float32';
    if (this.data instanceof Int32Array) return 'int32';
    return 'object';
  }
  get T() {   // transposes the last two axes (copy), like nd_array.js:362-366
    const sh = Int32Array.from(this.shape), n = sh.length;
    if (n < 2) return this;
    const [M, N] = [sh[n - 2], sh[n - 1]]; sh[n - 2] = N; sh[n - 1] = M;
    const out = new this.data.constructor(this.data.length);
    for (let o = 0; o < out.length; o += M * N)
      for (let i = 0; i < M; i++) for (let j = 0; j < N; j++) out[o + j * M + i] = this.data[o + i * N + j];
    return new NDArray(sh, out);
  }
}
function fromNested(a) {           // nested JS arrays -> NDArray(float64)  (asarray, nd_array.js:102-126)
  const shape = [];
  for (let x = a; Array.isArray(x); x = x[0]) shape.push(x.length);
  const data = new Float64Array(shape.reduce((p, q) => p * q, 1));
  let k = 0;
  (function walk(x, d) {
    if (d === shape.length) { data[k++] = +x; return; }
    if (!Array.isArray(x) || x.length !== shape[d]) throw new Error('asarray(): ragged nested array.');
    for (const y of x) walk(y, d + 1);
  })(a, 0);
  return new NDArray(Int32Array.from(shape.length ? shape : [1]), data);
}
/* ---- planners of the strided N-d copy (csrc/gather.hip): sliceElems (nd_array.js:531-642), transpose(...axes) (nd_array.js:375-436),
 * reshape (nd_array.js:438-462), concat (concat.js) and stack (stack.js) on shapes alone. Own code with the reference's messages;
 * twins of nd4js_amd/la.py's _slice_plan ... _reduce_box. Offsets and strides are in elements of a row-major operand. ---- */
function cStrides(shape) {
  const st = new Array(shape.length); let s = 1;
  for (let d = shape.length - 1; d >= 0; d--) { st[d] = s; s *= shape[d]; }
  return st;
}
function checkShape(shape, n) {                  // the NDArray constructor's two checks
  if (shape.some(s => s < 1)) throw new Error(`Invalid shape: ${shape.join(',')}.`);
  if (n !== shape.reduce((a, b) => a * b, 1)) throw new Error(`Shape [${shape.join(',')}] does not match array length of ${n}.`);
}
// -> {shape, off, strides}: out[i] = data[off + sum i_d strides[d]]
function slicePlan(shape, slices) {
  shape = Array.from(shape); slices = Array.from(slices);
  const ndim = shape.length;
  let nEll = 0, nRed = 0, nSl = 0;
  for (const s of slices) {
    if (s === '...') nEll++;
    else if (s === 'new') continue;
    else if (typeof s === 'number') { if (!(s % 1 === 0)) throw new Error('Only integral indices allowed.'); nRed++; }
    else {
      const len = s == null ? undefined : s.length;
      if (typeof len !== 'number' || !(len % 1 === 0) || len > 3 || len === 1) throw new Error('Illegal argument(s).');
      nSl++;
    }
  }
  if (nEll > 1) throw new Error('Highlander! There can be only one ... (ellipsis).');
  if (nEll === 0) slices.push('...');
  if (nRed + nSl > ndim) throw new Error('Cannot sliced more dimensions than available.');
  let off = 0, d = ndim, stride = 1;
  const out = [], strides = [];                  // innermost first
  for (let k = slices.length; --k >= 0;) {
    const s = slices[k];
    if (s === 'new') { strides.push(0); out.push(1); continue; }
    if (s === '...') { for (let i = nRed + nSl; i < ndim; i++) { d--; strides.push(stride); out.push(shape[d]); stride *= shape[d]; } continue; }
    const n = shape[--d];
    if (typeof s === 'number') {
      const i = s < 0 ? s + n : s;
      if (i < 0 || i >= n) throw new Error('Index out of bounds.');
      off += stride * i;
    } else {
      let start = s[0] == null ? null : +s[0], end = s[1] == null ? null : +s[1];
      const step = s[2] == null ? 1 : +s[2];
      if (end !== null && end < 0) end += n;
      if (start !== null && start < 0) start += n;
      if (start !== null && (start < 0 || start >= n)) throw new Error('Slice start out of bounds.');
      if (step === 0) throw new Error('Stride/step cannot be zero.');
      if (step < 0) {
        if (start === null) start = n - 1;
        if (end === null) end = -1;
        if (end < -1 || end >= n) throw new Error('Slice end out of bounds.');
      } else {
        if (start === null) start = 0;
        if (end === null) end = n;
        if (end < 0 || end > n) throw new Error('Slice end out of bounds.');
      }
      strides.push(stride * step);
      off += stride * start;
      out.push(1 + Math.trunc((-Math.sign(step) + end - start) / step));
    }
    stride *= n;
  }
  out.reverse(); strides.reverse();
  const count = out.reduce((a, b) => a * b, 1);
  if (count < 0) throw new Error(`Invalid typed array length: ${count}`);      // an empty range the wrong way round: the engine's text
  if (out.some(x => x < 1)) throw new Error(`Invalid shape: ${out.join(',')}.`);
  return {shape: out, off, strides};
}
// -> {shape, strides}; no axes: the last two swapped; axes that are not named follow the named ones in their own order
function transposePlan(shape, axes) {
  shape = Array.from(shape); axes = Array.from(axes);
  const ndim = shape.length, old = cStrides(shape);
  let order;
  if (axes.length === 0) { order = shape.map((_, i) => i); if (ndim > 1) { order[ndim - 2] = ndim - 1; order[ndim - 1] = ndim - 2; } }
  else {
    const set = new Set(axes);
    if (set.size !== axes.length) throw new Error('Duplicate axes are not allowed.');
    if (axes.some(j => !(j >= 0 && j < ndim))) throw new Error('Axis out of bounds.');
    order = axes.concat(shape.map((_, i) => i).filter(i => !set.has(i)));
  }
  return {shape: order.map(j => shape[j]), strides: order.map(j => old[j])};
}
// the new shape of an array of n elements, one -1 inferred
function reshapeShape(shape, n, newShape) {
  newShape = Array.from(Int32Array.from(newShape));
  let rest = 1, infer = -1;
  for (let i = newShape.length; --i >= 0;)
    if (newShape[i] < 0) {
      if (newShape[i] !== -1) throw new Error('Invalid dimension: ' + newShape[i]);
      if (infer !== -1) throw new Error('At most on dimension may be -1.');
      infer = i;
    } else rest *= newShape[i];
  if (infer !== -1) {
    if (0 !== n % rest) throw new Error('Shape cannot be inferred.');          // (n % 0 is NaN: refused as well)
    newShape[infer] = n / rest;
  }
  checkShape(newShape, n);
  return newShape;
}
// -> {shape, strides, offs}: piece k, read in its own row-major order, lands at out[offs[k] + sum i_d strides[d]]
function concatPlan(axis, shapes) {
  shapes = shapes.map(s => Array.from(s));
  if (axis == null) axis = 0;
  const ndim = shapes[0].length;
  if (0 > axis) axis += ndim;
  if (0 > axis || axis >= ndim) throw new Error('Axis out of bounds.');
  const out = shapes[0].slice();
  for (let i = shapes.length; --i > 0;) {
    const sh = shapes[i];
    if (out.length !== sh.length) throw new Error('All shapes must have the same length.');
    if (!out.every((len, d) => len === sh[d] || axis === d)) throw new Error('Shape along all axes but the concatentation axis must match.');
    out[axis] += sh[axis];
  }
  const strides = cStrides(out), offs = [];
  let at = 0;
  for (const sh of shapes) { offs.push(at * strides[axis]); at += sh[axis]; }
  return {shape: out, strides, offs};
}
// -> {axis, shapes (with the new axis of extent 1), shape, strides, offs}
function stackPlan(axis, shapes) {
  shapes = shapes.map(s => Array.from(s));
  if (axis == null) axis = 0;
  if (0 > axis) axis += shapes[0].length + 1;
  if (0 > axis || axis > shapes[0].length) throw new Error('Axis out of bounds.');
  const wide = shapes.map(s => s.slice(0, axis).concat([1], s.slice(axis)));
  return Object.assign({axis, shapes: wide}, concatPlan(axis, wide));
}
const GATHER_MAX_ND = 8;
// -> {shape, ss, ds, loop}: extent-1 axes dropped, neighbours merged where stride_d == stride_{d+1} shape_{d+1} on both sides, what
// exceeds GATHER_MAX_ND axes peeled off the outer end into a loop of [src offset, dst offset] pairs, one launch each
function reduceBox(shape, ss, ds) {
  const merged = [];
  for (let d = 0; d < shape.length; d++) {
    const n = shape[d], s = ss[d], t = ds[d];
    if (n === 1) continue;
    const last = merged[merged.length - 1];
    if (last && last[1] === s * n && last[2] === t * n) { last[0] *= n; last[1] = s; last[2] = t; }
    else merged.push([n, s, t]);
  }
  const cut = Math.max(0, merged.length - GATHER_MAX_ND), kept = merged.slice(cut);
  let loop = [[0, 0]];
  for (const [n, s, t] of merged.slice(0, cut)) {
    const next = [];
    for (const [a, b] of loop) for (let i = 0; i < n; i++) next.push([a + i * s, b + i * t]);
    loop = next;
  }
  return {shape: kept.map(a => a[0]), ss: kept.map(a => a[1]), ds: kept.map(a => a[2]), loop};
}
// one planned copy between device buffers; pairs: complex128, one more innermost axis of two 8-byte words
function gatherBox(dst, dstOff, dstStrides, src, srcOff, srcStrides, shape, pairs) {
  const eb = src.Ctor.BYTES_PER_ELEMENT;
  let sh = Array.from(shape), ss = Array.from(srcStrides), ds = Array.from(dstStrides);
  if (pairs) { sh.push(2); ss = ss.map(x => 2 * x).concat([1]); ds = ds.map(x => 2 * x).concat([1]); srcOff *= 2; dstOff *= 2; }
  const box = reduceBox(sh, ss, ds);
  for (const [so, dof] of box.loop) native().gather_nd(eb, box.shape, src.view(0), srcOff + so, box.ss, dst.view(0), dstOff + dof, box.ds);
}
/* ---- planners of the elementwise kernels (csrc/elem.hip): zip_elems' broadcast rule (zip_elems.js:43-53) and reduceElems' axes
 * (nd_array.js:479-497) on shapes alone, with the reference's messages; twins of la.py's _zip_plan and _reduce_plan. ---- */
const EW_OPS = {add: 0, sub: 1, mul: 2, div: 3, min: 4, max: 5, neg: 16, abs: 17};
const EW_ARITY = {add: 2, sub: 2, mul: 2, div: 2, min: 2, max: 2, neg: 1, abs: 1};
const EW_REDUCERS = ['add', 'mul', 'min', 'max'];
const EW_MAX_ND = 8;
// -> {shape, strides (per operand, 0 = broadcast), box: {shape, strides, loop}}: the box is reduced for the kernel (extent-1 axes
// dropped, neighbours merged where every operand allows) and what exceeds EW_MAX_ND axes is peeled off the outer end into a loop
// of [offset of each operand ..., offset in the result]
function zipPlan(shapes) {
  shapes = shapes.map(s => Array.from(s));
  const ndim = shapes.reduce((n, s) => Math.max(n, s.length), 0), shape = new Array(ndim).fill(1);
  for (const sh of shapes)
    for (let i = ndim, j = sh.length; i-- > 0 && j-- > 0;)
      if (1 === shape[i]) shape[i] = sh[j];
      else if (shape[i] !== sh[j] && sh[j] !== 1) throw new Error('Shapes are not broadcast-compatible.');
  const strides = shapes.map(sh => { const own = cStrides(sh), pad = ndim - sh.length; return shape.map((_, d) => d < pad || sh[d - pad] === 1 ? 0 : own[d - pad]); });
  const cs = cStrides(shape), merged = [];
  for (let d = 0; d < ndim; d++) {
    if (shape[d] === 1) continue;
    const ax = [shape[d], cs[d], ...strides.map(st => st[d])], last = merged[merged.length - 1];
    if (last && ax.every((s, k) => k === 0 || last[k] === s * ax[0])) { ax[0] *= last[0]; merged[merged.length - 1] = ax; }
    else merged.push(ax);
  }
  const cut = Math.max(0, merged.length - EW_MAX_ND), kept = merged.slice(cut);
  let loop = [new Array(shapes.length + 1).fill(0)];
  for (const ax of merged.slice(0, cut)) {
    const steps = ax.slice(2).concat([ax[1]]), next = [];
    for (const offs of loop) for (let i = 0; i < ax[0]; i++) next.push(offs.map((o, k) => o + i * steps[k]));
    loop = next;
  }
  return {shape, strides, box: {shape: kept.map(ax => ax[0]), strides: shapes.map((_, k) => kept.map(ax => ax[2 + k])), loop}};
}
// -> {shape, box: {shape, flags, loop}}: kept (0) and reduced (1) axes alternate in the box; kept axes beyond EW_MAX_ND are peeled off
// the outer end into a loop of [offset in the operand, offset in the result]. axes: a number, an iterable or a 1-D int32 NDArray.
function reducePlan(shape, axes) {
  shape = Array.from(shape);
  const ndim = shape.length;
  if ('number' === typeof axes) axes = [axes];
  else if (axes != null && axes.shape instanceof Int32Array && axes.data !== undefined) {
    const dt = dtypeOf(axes);
    if (dt !== 'int32') throw new Error(`Invalid dtype ${dt} for axes.`);
    if (axes.shape.length !== 1) throw new Error('Only 1D nd.Array allowed for axes.');
    axes = axes.data;
  }
  const red = new Set();
  for (let ax of axes) {
    if (0 > ax) ax += ndim;
    if (0 > ax || ax >= ndim) throw new Error('Reduction axis ' + ax + ' out of bounds.');
    red.add(+ax);
  }
  const merged = [];
  shape.forEach((n, d) => {
    if (n === 1) return;
    const f = red.has(d) ? 1 : 0, last = merged[merged.length - 1];
    if (last && last[1] === f) last[0] *= n; else merged.push([n, f]);
  });
  let loop = [[0, 0]];
  while (merged.length > EW_MAX_ND && merged[0][1] === 0) {
    const n = merged.shift()[0], aStep = merged.reduce((p, m) => p * m[0], 1), cStep = merged.reduce((p, m) => m[1] ? p : p * m[0], 1), next = [];
    for (const [a, c] of loop) for (let i = 0; i < n; i++) next.push([a + i * aStep, c + i * cStep]);
    loop = next;
  }
  if (merged.length > EW_MAX_ND) throw new Error(`reduceElems: more than ${EW_MAX_ND} alternating kept and reduced axes are not accelerated.`);
  return {shape: shape.filter((_, d) => !red.has(d)), box: {shape: merged.map(m => m[0]), flags: merged.map(m => m[1]), loop}};
}
/* The operators as closures, for standalone use (after install(nd) the host module's own nd.math members are recognised as well):
 * on float64 each is one IEEE operation, which is what the device runs. A closure is recognised by identity, never by its text. */
const math = Object.freeze({
  add: (x, y) => x + y, sub: (x, y) => x - y, mul: (x, y) => x * y, div: (x, y) => x / y,
  min: (x, y) => Math.min(x, y), max: (x, y) => Math.max(x, y), neg: x => -x, abs: x => Math.abs(x),
});
const mathTables = [math];                       // install(nd) adds nd.math
// the operator name behind `fn` (a name, or a function identical to a member of a known math table), or null
function ewName(fn) {
  if (typeof fn === 'string') return Object.prototype.hasOwnProperty.call(EW_OPS, fn) ? fn : null;
  if (typeof fn !== 'function') return null;
  for (const t of mathTables) for (const k of Object.keys(EW_OPS)) if (t[k] === fn) return k;
  return null;
}
// C = op(A, B) on device buffers (B null: unary), planned by zipPlan; returns the fresh buffer
function zipBox(op, plan, bufs) {
  const n = plan.shape.reduce((a, b) => a * b, 1), C = new DevBuf(n, Float64Array), b = plan.box;
  try {
    for (const offs of b.loop)
      native().zip_nd(EW_OPS[op], b.shape, bufs[0].view(0), offs[0], b.strides[0], bufs.length > 1 ? bufs[1].view(0) : null,
                      bufs.length > 1 ? offs[1] : 0, bufs.length > 1 ? b.strides[1] : [], C.view(offs[offs.length - 1]));
  } catch (e) { C.free(); throw e; }
  return C;
}
/* ---- device-resident arrays (SURVEY.md §8f N3): `data` stays in HBM across calls, lazy D2H on `.data` ----
 * An extension of the NDArray contract (nd_array.js:128-158), not part of the reference: any nd.la hot-path function
 * that receives at least one DeviceNDArray runs the `_dev` entry points (nothing crosses PCIe except host operands
 * uploaded on the way in) and returns DeviceNDArrays. Results are immutable, so the host copy is cached. */
class DevBuf {
  constructor(length, Ctor) {
    this.length = length; this.Ctor = Ctor;
    this.ext = native().dev_alloc(length * Ctor.BYTES_PER_ELEMENT);
  }
  static from(typed) { const b = new DevBuf(typed.length, typed.constructor); native().dev_upload(b.ext, 0, typed); return b; }
  view(off) { if (!this.ext) throw new Error('nd4hip: device array was disposed.'); return {b: this.ext, o: off}; }
  free() { if (this.ext) { native().dev_free(this.ext); this.ext = null; } }
}
/* A host-module complex array over the interleaved (re, im) doubles `f64`, without a copy: the reference's ComplexArray constructor
 * is (buffer, byteOffset, length in complex elements), src/dt/complex_array.js, and keeps the doubles as `_array`. */
const complexOver = (Complex, f64) => new Complex(f64.buffer, f64.byteOffset, f64.length / 2);
/* complex128: `Complex` is the host module's Complex128Array class; the buffer holds 2n doubles, interleaved (re, im) as
 * the reference's ComplexArray._array, and `.data` is a Complex128Array over the downloaded Float64Array. */
class DeviceNDArray {
  constructor(shape, buf, Complex) {
    if (!(shape instanceof Int32Array)) throw new Error('Shape must be Int32Array.');
    const n = shape.reduce((a, b) => a * b, 1);
    if (!(buf instanceof DevBuf) || buf.length !== (Complex ? 2 * n : n)) throw new Error(`Shape [${shape}] does not match the device buffer.`);
    if (Complex && buf.Ctor !== Float64Array) throw new Error('nd4hip: a complex128 device array is stored as float64 pairs.');
    this.shape = shape; this._buf = buf; this._host = null; this._complex = Complex || null;
  }
  get ndim() { return this.shape.length; }
  get dtype() { return this._complex ? 'complex128' : this._buf.Ctor === Int32Array ? 'int32' : 'float64'; }
  get onDevice() { return true; }
  get data() {                                   // lazy D2H (blocks until everything queued before it has finished)
    if (this._host === null) {
      if (!this._buf.ext) throw new Error('nd4hip: device array was disposed.');
      const h = new this._buf.Ctor(this._buf.length);
      native().dev_download(h, this._buf.ext, 0);
      this._host = this._complex ? complexOver(this._complex, h) : h;
    }
    return this._host;
  }
  /* NDArray.T (nd_array.js): a new device array with the last two axes swapped, transposed on the device (csrc/struct.hip);
   * fewer than two axes: this array itself. float64 only. */
  static transposedShape(shape, dtype) {          // the rules of .T without a device: null = the array itself
    const nd_ = shape.length;
    if (nd_ < 2) return null;
    if (dtype !== 'float64') throw new Error(`nd4hip.T: ${dtype} device arrays are not accelerated.`);
    const out = Int32Array.from(shape);
    out[nd_ - 2] = shape[nd_ - 1]; out[nd_ - 1] = shape[nd_ - 2];
    return out;
  }
  get T() {
    const nd_ = this.ndim, shape = DeviceNDArray.transposedShape(this.shape, this.dtype);
    if (shape === null) return this;
    const M = this.shape[nd_ - 2], N = this.shape[nd_ - 1];
    const B = new DevBuf(this._buf.length, Float64Array);
    native().dtranspose_batched(this._buf.length / (M * N || 1), M, N, this._buf.view(0), B.view(0));
    return new DeviceNDArray(shape, B);
  }
  /* NDArray.sliceElems / transpose(...axes) / reshape on the device (csrc/gather.hip): float64, int32 and complex128. sliceElems and
   * transpose with axes return fresh device arrays; transpose() without axes is .T and keeps .T's rules. reshape returns a device
   * array over the SAME buffer, as the reference's reshape shares `data`: dispose() on either one releases both. */
  sliceElems(...slices) {
    const p = slicePlan(this.shape, slices), pairs = !!this._complex;
    const B = new DevBuf(p.shape.reduce((a, b) => a * b, 1) * (pairs ? 2 : 1), this._buf.Ctor);
    gatherBox(B, 0, cStrides(p.shape), this._buf, p.off, p.strides, p.shape, pairs);
    return new DeviceNDArray(Int32Array.from(p.shape), B, this._complex);
  }
  transpose(...axes) {
    if (axes.length === 0) return this.T;
    const p = transposePlan(this.shape, axes), pairs = !!this._complex;
    const B = new DevBuf(this._buf.length, this._buf.Ctor);
    gatherBox(B, 0, cStrides(p.shape), this._buf, 0, p.strides, p.shape, pairs);
    return new DeviceNDArray(Int32Array.from(p.shape), B, this._complex);
  }
  reshape(...shape) {
    const n = this.shape.reduce((a, b) => a * b, 1);
    if (!this._buf.ext) throw new Error('nd4hip: device array was disposed.');
    return new DeviceNDArray(Int32Array.from(reshapeShape(this.shape, n, shape)), this._buf, this._complex);
  }
  /* NDArray.mapElems / reduceElems on the device (csrc/elem.hip), float64 only, for the closures that are one IEEE operation:
   * mapElems() and mapElems('float64') copy, mapElems('float64', neg | abs) computes; reduceElems(axes, 'float64', add | mul | min |
   * max) folds every output in the reference's order (sums and products have its bits). An operator is its name or a function
   * identical to the host module's nd.math member (or this package's `math`). Every other form throws: a device array is never
   * handed to a host closure. */
  mapElems(dtype, mapper) {
    if (typeof dtype === 'function' || (dtype == null && mapper != null)) throw new Error('nd4hip.mapElems: a mapper without dtype is not accelerated.');
    if ((dtype != null && dtype !== 'float64') || this.dtype !== 'float64') throw new Error('nd4hip.mapElems: dtype is not accelerated.');
    const n = this._buf.length;
    if (mapper == null) {
      const B = new DevBuf(n, Float64Array);
      gatherBox(B, 0, [1], this._buf, 0, [1], [n], false);
      return new DeviceNDArray(Int32Array.from(this.shape), B);
    }
    const op = ewName(mapper);
    if (op === null || EW_ARITY[op] !== 1) throw new Error('nd4hip.mapElems: mapper is not accelerated.');
    return new DeviceNDArray(Int32Array.from(this.shape), zipBox(op, zipPlan([this.shape]), [this._buf]));
  }
  reduceElems(axes, dtype, reducer) {
    if (reducer == null) throw new Error('nd4hip.reduceElems: the forms without (axes, dtype, reducer) are not accelerated.');
    if (dtype !== 'float64' || this.dtype !== 'float64') throw new Error('nd4hip.reduceElems: dtype is not accelerated.');
    const op = ewName(reducer);
    if (op === null || !EW_REDUCERS.includes(op)) throw new Error('nd4hip.reduceElems: reducer is not accelerated.');
    const p = reducePlan(this.shape, axes), b = p.box;
    const C = new DevBuf(p.shape.reduce((x, y) => x * y, 1), Float64Array);
    try {
      for (const [ao, co] of b.loop) native().reduce_nd(EW_OPS[op], b.shape, b.flags, this._buf.view(ao), C.view(co));
    } catch (e) { C.free(); throw e; }
    return new DeviceNDArray(Int32Array.from(p.shape), C);
  }
  toHost(NDA) { return new (NDA || NDArray)(Int32Array.from(this.shape), this.data); }
  dispose() { this._buf.free(); }                // optional: dropped arrays are freed by the GC finalizer
}
const isDev = a => a instanceof DeviceNDArray;
const isComplexDev = a => isDev(a) && a.dtype === 'complex128';
/* singular_matrix_solve_error.js: thrown by rrqr_solve / solve of a rank-deficient system, `.x` = the least-squares solution.
 * Standalone this class is thrown; after install(nd) the host module's own nd.la.SingularMatrixSolveError is. */
class SingularMatrixSolveError extends Error {
  constructor(x, ...args) { super(...args); this.x = x; }
}

function makeAsarray(NDA) {
  return function asarray(a) {
    if (isDev(a)) return a;                                                       // never touches .data (no D2H)
    if (a && a.shape instanceof Int32Array && a.data !== undefined) return a;     // NDArray of either package
    if (Array.isArray(a)) { const r = fromNested(a); return NDA === NDArray ? r : new NDA(r.shape, r.data); }
    if (typeof a === 'number') return new NDA(Int32Array.of(1), Float64Array.of(a));
    throw new Error('asarray(): unsupported argument.');
  };
}
const dtypeOf = a => isDev(a) ? a.dtype : a.data instanceof Float64Array ? 'float64' : a.data instanceof Int32Array ? 'int32' :
  a.data instanceof Float32Array ? 'float32' : (a.dtype || 'object');
const f64 = a => a.data instanceof Float64Array ? a.data : Float64Array.from(a.data);    // int32 -> float64 promotion
const prod = (s, from, to) => { let p = 1; for (let i = from; i < to; i++) p *= s[i]; return p; };

/* Flatten NumPy-style broadcasting of the leading axes into (count, offA, strideA, offB, strideB, offC)
 * groups with batch strides in {0, dense}: the job of the odometer at matmul.js:44-70. */
function bcastGroups(lead, la, lb, IK, KJ) {
  const nb = lead.length, pad = (s) => Array(nb - s.length).fill(1).concat(Array.from(s));
  la = pad(la); lb = pad(lb);
  const strides = (sh, unit) => { const st = Array(nb).fill(0); let s = unit; for (let d = nb - 1; d >= 0; d--) { st[d] = sh[d] > 1 ? s : 0; s *= sh[d]; } return st; };
  const stA = strides(la, IK), stB = strides(lb, KJ), total = lead.reduce((a, b) => a * b, 1);
  const offA = new Float64Array(total), offB = new Float64Array(total), idx = Array(nb).fill(0);
  for (let b = 0; b < total; b++) {
    let a = 0, c = 0; for (let d = 0; d < nb; d++) { a += idx[d] * stA[d]; c += idx[d] * stB[d]; }
    offA[b] = a; offB[b] = c;
    for (let d = nb - 1; d >= 0; d--) { if (++idx[d] < lead[d]) break; idx[d] = 0; }
  }
  const groups = [];
  for (let b0 = 0; b0 < total;) {
    let b1 = b0 + 1, sA = 0, sB = 0;
    if (b1 < total) {
      sA = offA[b1] - offA[b0]; sB = offB[b1] - offB[b0];
      if ((sA === 0 || sA === IK) && (sB === 0 || sB === KJ))
        while (b1 < total && offA[b1] - offA[b1 - 1] === sA && offB[b1] - offB[b1 - 1] === sB) b1++;
      else sA = sB = 0;
    }
    groups.push([b1 - b0, offA[b0], sA, offB[b0], sB, b0]);
    b0 = b1;
  }
  return groups;
}

/* n-operand form of bcastGroups: [count, [offsets], [strides], outIndex] with stride_k in {0, units[k]} */
function bcastGroupsN(lead, shapes, units) {
  const nb = lead.length, total = lead.reduce((a, b) => a * b, 1);
  const offs = shapes.map((sh, k) => {
    const s = Array(nb - sh.length).fill(1).concat(Array.from(sh)), st = Array(nb).fill(0);
    let u = units[k]; for (let d = nb - 1; d >= 0; d--) { st[d] = s[d] > 1 ? u : 0; u *= s[d]; }
    const o = new Float64Array(total), idx = Array(nb).fill(0);
    for (let b = 0; b < total; b++) {
      let a = 0; for (let d = 0; d < nb; d++) a += idx[d] * st[d];
      o[b] = a;
      for (let d = nb - 1; d >= 0; d--) { if (++idx[d] < lead[d]) break; idx[d] = 0; }
    }
    return o;
  });
  const groups = [];
  for (let b0 = 0; b0 < total;) {
    let b1 = b0 + 1, strides = units.map(() => 0);
    if (b1 < total) {
      const cand = offs.map(o => o[b1] - o[b0]);
      if (cand.every((c, k) => c === 0 || c === units[k])) {
        strides = cand;
        while (b1 < total && offs.every((o, k) => o[b1] - o[b1 - 1] === cand[k])) b1++;
      }
    }
    groups.push([b1 - b0, offs.map(o => o[b0]), strides, b0]);
    b0 = b1;
  }
  return groups;
}
/* Common shape of right-aligned leading-axis lists under NumPy broadcasting (extent 1 stretches). */
function bcastLead(shapes, err) {
  const rank = shapes.reduce((r, sh) => Math.max(r, sh.length), 0), lead = new Array(rank).fill(1);
  shapes.forEach(sh => {
    const shift = rank - sh.length;
    for (let d = 0; d < sh.length; d++) {
      const have = lead[shift + d], want = sh[d];
      if (want === 1 || want === have) continue;
      if (have !== 1) throw new Error(err);
      lead[shift + d] = want;
    }
  });
  return lead;
}
/* Shape of matmul2 for operand shapes sA, sB (plain arrays / Int32Arrays): [result shape, I, K, J]. */
function productShape(sA, sB, mismatch) {
  const I = sA[sA.length - 2], K = sA[sA.length - 1], J = sB[sB.length - 1];
  if (sB[sB.length - 2] != K) throw new Error(mismatch);
  const lead = bcastLead([Array.from(sA).slice(0, -2), Array.from(sB).slice(0, -2)], 'Shapes are not broadcast-compatible.');
  return [lead.concat([I, J]), I, K, J];
}

function makeLa(NDA, fallback, SolveError, Complex) {
  const asarray = makeAsarray(NDA);
  const gpuOk = a => { const d = dtypeOf(a); return d === 'float64' || d === 'int32'; };
  const la = {};
  /* residency plumbing: one code path per function, host TypedArrays or device buffers */
  const alloc = (dev, n, Ctor) => dev ? new DevBuf(n, Ctor || Float64Array) : new (Ctor || Float64Array)(n);
  const view = (x, off) => x instanceof DevBuf ? x.view(off) : x.subarray(off);
  const wrap = (dev, shape, x) => dev ? new DeviceNDArray(Int32Array.from(shape), x) : new NDA(Int32Array.from(shape), x);
  const opF64 = (a, dev, temps) => {             // operand storage as float64 on the side the call runs on
    if (!dev) return f64(a);
    if (isDev(a) && a.dtype === 'float64') return a._buf;
    const b = DevBuf.from(f64(a)); temps.push(b); return b;      // host operand (or device int32): upload a float64 copy
  };
  const opI32 = (a, dev, temps) => {
    if (!dev) return a.data;
    if (isDev(a)) return a._buf;
    const b = DevBuf.from(a.data); temps.push(b); return b;
  };
  const release = temps => { for (const t of temps) t.free(); };
  la.DeviceNDArray = DeviceNDArray;
  la.to_device = a => { a = asarray(a); if (isDev(a)) return a;
                        if (dtypeOf(a) === 'complex128') { const Cx = needComplex('to_device'); return new DeviceNDArray(Int32Array.from(a.shape), DevBuf.from(a.data._array), Cx); }
                        if (!gpuOk(a)) throw new Error('nd4hip.to_device: dtype ' + dtypeOf(a) + ' is not accelerated.');
                        return new DeviceNDArray(Int32Array.from(a.shape), DevBuf.from(a.data)); };
  la.to_host = a => isDev(a) ? a.toHost(NDA) : asarray(a);
  la.synchronize = () => native().synchronize();
  // per-call profile of the C ABI (nd4hip_profile_enable / nd4hip_profile_last): kernel ms, algorithmic flops and bytes per device
  la.profile_enable = on => native().profile_enable(on !== false);
  la.profile_last = () => native().profile_last();

  /* complex128 lives in the host module's Complex128Array; the standalone module has none */
  const needComplex = name => {
    if (!Complex) throw new Error(`nd4hip.${name}: complex128 needs the host nd4js module (install(nd)); the standalone module has no complex arrays.`);
    return Complex;
  };
  const opZ = (a, dev, temps) => {               // operand storage as doubles (complex: interleaved re, im) on the call's side
    if (dtypeOf(a) !== 'complex128') return opF64(a, dev, temps);
    if (isDev(a)) return a._buf;
    if (!dev) return a.data._array;
    const b = DevBuf.from(a.data._array); temps.push(b); return b;
  };
  /* matmul2_CC / _CR / _RC (matmul.js:74-87): zgemm_batched; strides count elements, buffer offsets count doubles */
  const zmatmul2 = (a, b, shape, I, K, J) => {
    const Cx = needComplex('matmul2');
    const ac = dtypeOf(a) === 'complex128', bc = dtypeOf(b) === 'complex128', ea = ac ? 2 : 1, eb = bc ? 2 : 1;
    const lead = shape.slice(0, -2), n = shape.reduce((m, k) => m * k, 1);
    const dev = isDev(a) || isDev(b), temps = [];
    const A = opZ(a, dev, temps), B = opZ(b, dev, temps), C = alloc(dev, 2 * n);
    try {
      for (const [cnt, offA, sA, offB, sB, offC] of bcastGroups(lead, a.shape.subarray(0, a.ndim - 2), b.shape.subarray(0, b.ndim - 2), I * K, K * J))
        native().zgemm_batched(ac ? 1 : 0, bc ? 1 : 0, cnt, I, K, J, view(A, ea * offA), sA, view(B, eb * offB), sB, view(C, 2 * offC * I * J));
    } finally { release(temps); }
    return dev ? new DeviceNDArray(Int32Array.from(shape), C, Cx) : new NDA(Int32Array.from(shape), complexOver(Cx, C));
  };

  la.matmul2 = function matmul2(a, b) {
    a = asarray(a); b = asarray(b);
    if (a.ndim < 2) throw new Error('A must be at least 2D.');
    if (b.ndim < 2) throw new Error('B must be at least 2D.');
    const [shape, I, K, J] = productShape(a.shape, b.shape, 'The last dimension of A and the 2nd to last dimension of B do not match.');
    const da = dtypeOf(a), db = dtypeOf(b);
    // complex128 with complex128, float64 or int32 (either order): result complex128, the reference's products
    if ((da === 'complex128' && (db === 'complex128' || gpuOk(b))) || (db === 'complex128' && gpuOk(a))) return zmatmul2(a, b, shape, I, K, J);
    // GPU path: at least one float64 operand and the other float64/int32 (result dtype float64, matmul.js:119);
    // int32 x int32 (wrapping Int32Array result), float32, complex128, object -> the host's own function
    if (!((da === 'float64' && gpuOk(b)) || (db === 'float64' && gpuOk(a)))) {
      if (fallback && fallback.matmul2) return fallback.matmul2(a, b);
      throw new Error(`nd4hip.matmul2: dtype pair (${da}, ${db}) is not accelerated and no host nd4js was installed.`);
    }
    const lead = shape.slice(0, -2);
    const dev = isDev(a) || isDev(b), temps = [];
    const A = opF64(a, dev, temps), B = opF64(b, dev, temps), C = alloc(dev, shape.reduce((m, n) => m * n, 1));
    for (const [cnt, offA, sA, offB, sB, offC] of bcastGroups(lead, a.shape.subarray(0, a.ndim - 2), b.shape.subarray(0, b.ndim - 2), I * K, K * J))
      native().dgemm_batched(cnt, I, K, J, view(A, offA), sA, view(B, offB), sB, view(C, offC * I * J));
    release(temps);
    return wrap(dev, shape, C);
  };

  /* Matrix-chain ordering (CLRS 15.2) with broadcast leading axes; one product costs numel(result)*K, which is how
     matmul.js:150-236 counts. cut[lo][hi] = last operand of the left factor of the cheapest split of lo..hi, the first
     among equals. A sub-chain's shape does not depend on its split, so one shape per span is kept. */
  la._chain_plan = function chainPlan(shapes) {
    const n = shapes.length, table = init => shapes.map(() => new Array(n).fill(init));
    const span = table(null), cost = table(0), cut = table(-1);
    shapes.forEach((sh, k) => { span[k][k] = Array.from(sh); });
    for (let width = 1; width < n; width++)
      for (let lo = 0, hi = width; hi < n; lo++, hi++) {
        let best = Infinity;
        for (let mid = lo; mid < hi; mid++) {
          const [shp, , K] = productShape(span[lo][mid], span[mid + 1][hi], 'Shape mismatch.');
          const c = shp.reduce((v, e) => v * e, 1) * K + (cost[lo][mid] + cost[mid + 1][hi]);
          if (c < best) { best = c; cut[lo][hi] = mid; span[lo][hi] = shp; }
        }
        if (cut[lo][hi] < 0) throw new Error('Integer overflow (too many FLOPs).');
        cost[lo][hi] = best;
      }
    return cut;
  };
  la.matmul = function matmul(...matrices) {            // contract of matmul.js:150-236; the ordering stays on the host
    const ms = matrices.map(asarray);
    if (ms.length === 1) return ms[0];
    if (ms.length === 2) return la.matmul2(ms[0], ms[1]);
    const cut = la._chain_plan(ms.map(m => m.shape));
    const evaluate = (lo, hi) => lo === hi ? ms[lo] : la.matmul2(evaluate(lo, cut[lo][hi]), evaluate(cut[lo][hi] + 1, hi));
    return evaluate(0, ms.length - 1);
  };

  la.qr_decomp = function qr_decomp(A) {
    A = asarray(A);
    if (A.ndim < 2) throw new Error('qr_decomp(A): A.ndim must be at least 2.');
    if (!gpuOk(A)) { if (fallback && fallback.qr_decomp) return fallback.qr_decomp(A); throw new Error('nd4hip.qr_decomp: dtype ' + dtypeOf(A) + ' is not accelerated.'); }
    const nd_ = A.ndim, M = A.shape[nd_ - 2], N = A.shape[nd_ - 1], L = Math.min(M, N), batch = prod(A.shape, 0, nd_ - 2);
    const Qs = Int32Array.from(A.shape), Rs = Int32Array.from(A.shape); Qs[nd_ - 1] = L; Rs[nd_ - 2] = L;
    const dev = isDev(A), temps = [];
    const Q = alloc(dev, batch * M * L), R = alloc(dev, batch * L * N);
    native().dgeqrf_q_batched(batch, M, N, view(opF64(A, dev, temps), 0), view(Q, 0), view(R, 0));
    release(temps);
    return [wrap(dev, Qs, Q), wrap(dev, Rs, R)];
  };

  la.qr_decomp_full = function qr_decomp_full(A) {         // qr.js:27-77: Q [..., M, M], R [..., M, N]
    A = asarray(A);
    if (A.ndim < 2) throw new Error('A must be at least 2D.');
    if (!gpuOk(A)) { if (fallback && fallback.qr_decomp_full) return fallback.qr_decomp_full(A); throw new Error('nd4hip.qr_decomp_full: dtype ' + dtypeOf(A) + ' is not accelerated.'); }
    const nd_ = A.ndim, M = A.shape[nd_ - 2], N = A.shape[nd_ - 1], batch = prod(A.shape, 0, nd_ - 2);
    const Qs = Int32Array.from(A.shape); Qs[nd_ - 1] = M;
    const dev = isDev(A), temps = [];
    const Q = alloc(dev, batch * M * M), R = alloc(dev, batch * M * N);
    native().dgeqrf_full_batched(batch, M, N, view(opF64(A, dev, temps), 0), view(Q, 0), view(R, 0));
    release(temps);
    return [wrap(dev, Qs, Q), wrap(dev, A.shape, R)];
  };

  /* qr.js:146-183, same signature and in-place semantics: A (M x N at A_off) <- R, Y (M x L at Y_off) <- Q^T Y.
     A and Y are Float64Arrays; the reference's assertions are kept (its only message is 'Assertion failed.'). */
  la._qr_decomp_inplace = function _qr_decomp_inplace(M, N, L, A, A_off, Y, Y_off) {
    for (const v of [M, N, L, A_off, Y_off]) if (v % 1 !== 0 || !(0 <= v)) throw new Error('Assertion failed.');
    if (!(A instanceof Float64Array) || !(Y instanceof Float64Array)) {
      if (fallback && fallback._qr_decomp_inplace) return fallback._qr_decomp_inplace(M, N, L, A, A_off, Y, Y_off);
      throw new Error('nd4hip._qr_decomp_inplace: only Float64Array storage is accelerated.');
    }
    if (!(M * N <= A.length - A_off)) throw new Error('Assertion failed.');
    if (!(M * L <= Y.length - Y_off)) throw new Error('Assertion failed.');
    if (M === 0 || N === 0) return;
    native().dgeqrf_qty_batched(1, M, N, L, A.subarray(A_off, A_off + M * N), Y.subarray(Y_off, Y_off + M * L));
  };

  la.lu_decomp = function lu_decomp(A) {
    A = asarray(A);
    const nd_ = A.ndim;
    if (nd_ < 2 || A.shape[nd_ - 2] != A.shape[nd_ - 1]) throw new Error('Last two dimensions must be quadratic.');
    if (!gpuOk(A)) { if (fallback && fallback.lu_decomp) return fallback.lu_decomp(A); throw new Error('nd4hip.lu_decomp: dtype ' + dtypeOf(A) + ' is not accelerated.'); }
    const N = A.shape[nd_ - 1], batch = prod(A.shape, 0, nd_ - 2);
    const dev = isDev(A), temps = [];
    const LU = alloc(dev, batch * N * N), P = alloc(dev, batch * N, Int32Array);
    native().dgetrf_batched(batch, N, view(opF64(A, dev, temps), 0), view(LU, 0), view(P, 0));
    release(temps);
    return [wrap(dev, A.shape, LU), wrap(dev, A.shape.subarray(0, nd_ - 1), P)];
  };

  // opts.algo: undefined / 'jacobi' (the default route) or 'dc' (bidiagonalisation + divide & conquer, svd_dc.js's own algorithm)
  la.svd_decomp = function svd_decomp(A, opts) {
    const algo = opts == null ? undefined : opts.algo;
    if (algo !== undefined && algo !== null && algo !== 'jacobi' && algo !== 'dc') throw new Error("svd_decomp(A, {algo}): algo must be 'jacobi' or 'dc'.");
    if (opts != null && opts.subset != null) {     // the selected triplets alone, csrc/bdsvdx.hip (not with 'jacobi')
      if (algo === 'jacobi') throw new Error("svd_decomp(A, {subset}): subset is not available with algo 'jacobi'.");
      return svdSubset('svd_decomp(A, {subset})', A, opts.subset, true);
    }
    A = asarray(A);
    if (String(dtypeOf(A)).startsWith('complex')) throw new Error('svd_dc(A): A.dtype must be float.');
    if (A.ndim < 2) throw new Error('svd_decomp(A): A.ndim must be at least 2.');
    if (!gpuOk(A)) { if (fallback && fallback.svd_decomp) return fallback.svd_decomp(A); throw new Error('nd4hip.svd_decomp: dtype ' + dtypeOf(A) + ' is not accelerated.'); }
    const nd_ = A.ndim, M = A.shape[nd_ - 2], N = A.shape[nd_ - 1], L = Math.min(M, N), batch = prod(A.shape, 0, nd_ - 2);
    const Us = Int32Array.from(A.shape), Vs = Int32Array.from(A.shape); Us[nd_ - 1] = L; Vs[nd_ - 2] = L;
    const dev = isDev(A), temps = [];
    const U = alloc(dev, batch * M * L), sv = alloc(dev, batch * L), V = alloc(dev, batch * L * N);
    if (algo === 'dc') native().dgesdd_batched(batch, M, N, view(opF64(A, dev, temps), 0), view(U, 0), view(sv, 0), view(V, 0));
    else la.last_svd_info = native().dgesvdj_batched(batch, M, N, view(opF64(A, dev, temps), 0), view(U, 0), view(sv, 0), view(V, 0));
    release(temps);
    return [wrap(dev, Us, U), wrap(dev, Vs.subarray(0, nd_ - 1), sv), wrap(dev, Vs, V)];
  };
  la.svd_dc = la.svd_decomp;

  /* ---- selected singular triplets, csrc/bdsvdx.hip (not in the reference): svd_decomp(A, {subset: [i0, i1]}) -> [U [..., M, k],
   * sv [..., k], V [..., k, N]] for sv[i0:i1] of the descending singular values; svd_vals(A, {subset}) -> sv alone (default: all),
   * the same bits; bidiag_svd(d, e, {subset}) -> [U2 [..., K, k], sv [..., k], V2 [..., k, J]] and bidiag_svdvals(d, e, {subset}) for
   * the upper bidiagonal K x J matrix (J = K or K + 1; e null for K = J = 1), default subset: all. min(M, N), K <= 2048. An empty
   * subset throws: an NDArray has no axis of length 0. Host arrays or DeviceNDArrays in, the same kind out. ---- */
  const subsetOf = (what, subset, L, bound) => {
    if (subset == null) return [0, L];
    const ok = (Array.isArray(subset) || ArrayBuffer.isView(subset)) && subset.length === 2;
    const [i0, i1] = ok ? subset : [NaN, NaN];
    if (!(ok && Number.isInteger(i0) && Number.isInteger(i1) && 0 <= i0 && i0 <= i1 && i1 <= L))
      throw new Error(`${what}: subset must be [i0, i1] with 0 <= i0 <= i1 <= ${bound}, got ${JSON.stringify(ok ? Array.from(subset) : subset)} for ${bound} = ${L}.`);
    if (i0 === i1) throw new Error(`${what}: the subset [${i0}, ${i1}] is empty, and an NDArray has no axis of length 0.`);
    return [i0, i1];
  };
  const svdSubset = (what, A, subset, vectors) => {
    A = asarray(A);
    if (isComplexDev(A) || String(dtypeOf(A)).startsWith('complex')) throw new TypeError(`${what}: A.dtype must be float.`);
    if (A.ndim < 2) throw new Error(`${what}: A.ndim must be at least 2.`);
    if (!gpuOk(A)) throw new TypeError(`${what}: dtype ${dtypeOf(A)} is not accelerated.`);
    const nd_ = A.ndim, M = A.shape[nd_ - 2], N = A.shape[nd_ - 1], L = Math.min(M, N), batch = prod(A.shape, 0, nd_ - 2);
    if (L > 2048) throw new Error(`${what}: min(M, N) <= 2048.`);
    const [i0, i1] = subsetOf(what, subset, L, 'min(M, N)'), k = i1 - i0, lead = Array.from(A.shape.subarray(0, nd_ - 2));
    const dev = isDev(A), temps = [], out = [];
    try {
      const sv = alloc(dev, batch * k); out.push(sv);
      const U = vectors ? alloc(dev, batch * M * k) : null; if (U) out.push(U);
      const V = vectors ? alloc(dev, batch * k * N) : null; if (V) out.push(V);
      native().dgesvdx_batched(batch, M, N, i0, i1, view(opF64(A, dev, temps), 0), U ? view(U, 0) : null, view(sv, 0), V ? view(V, 0) : null, null);
      const svw = wrap(dev, lead.concat([k]), sv);
      return vectors ? [wrap(dev, lead.concat([M, k]), U), svw, wrap(dev, lead.concat([k, N]), V)] : svw;
    }
    catch (err) { if (dev) for (const b of out) b.free(); throw err; }
    finally { release(temps); }
  };
  const svd_vals = function (A, opts) { return svdSubset('svd_vals(A)', A, opts == null ? undefined : opts.subset, false); };
  Object.defineProperty(la, 'svd_vals', {value: svd_vals, writable: true, enumerable: false, configurable: true});
  const bidiagSubset = (name, vectors) => {
    const f = function (d, e, opts) {
      const what = `${name}(d,e)`;
      d = asarray(d); e = e == null ? null : asarray(e);
      for (const X of e ? [d, e] : [d]) {
        if (isComplexDev(X) || String(dtypeOf(X)).startsWith('complex')) throw new TypeError(`${what}: the operands must be float.`);
        if (!gpuOk(X)) throw new TypeError(`${what}: dtype ${dtypeOf(X)} is not accelerated.`);
      }
      if (e && isDev(e) !== isDev(d)) throw new TypeError(`${what}: the operands must be all host arrays or all DeviceNDArrays.`);
      const nd_ = d.ndim, K = d.shape[nd_ - 1], lead = Array.from(d.shape.subarray(0, nd_ - 1)), J = e ? e.shape[e.ndim - 1] + 1 : 1;
      if ((J !== K && J !== K + 1) || (e && (e.ndim !== nd_ || lead.some((s, i) => s != e.shape[i]))))
        throw new Error(`${what}: e must have the leading dimensions of d and len(d) - 1 or len(d) entries (null for a 1 x 1 matrix).`);
      if (K > 2048) throw new Error(`${what}: K <= 2048.`);
      const [i0, i1] = subsetOf(what, opts == null ? undefined : opts.subset, K, 'K'), k = i1 - i0, batch = lead.reduce((p, q) => p * q, 1);
      const dev = isDev(d), temps = [], out = [];
      try {
        const sv = alloc(dev, batch * k); out.push(sv);
        const U2 = vectors ? alloc(dev, batch * K * k) : null; if (U2) out.push(U2);
        const V2 = vectors ? alloc(dev, batch * k * J) : null; if (V2) out.push(V2);
        native().dbdsvdx_batched(batch, K, J, i0, i1, view(opF64(d, dev, temps), 0), e ? view(opF64(e, dev, temps), 0) : null, U2 ? view(U2, 0) : null,
                                 view(sv, 0), V2 ? view(V2, 0) : null, null);
        const svw = wrap(dev, lead.concat([k]), sv);
        return vectors ? [wrap(dev, lead.concat([K, k]), U2), svw, wrap(dev, lead.concat([k, J]), V2)] : svw;
      }
      catch (err) { if (dev) for (const b of out) b.free(); throw err; }
      finally { release(temps); }
    };
    Object.defineProperty(f, 'name', {value: name});
    Object.defineProperty(la, name, {value: f, writable: true, enumerable: false, configurable: true});
  };
  bidiagSubset('bidiag_svd', true); bidiagSubset('bidiag_svdvals', false);

  /* ---- SURVEY §8f N1: solve-side consumers (csrc/trsm.hip) ---- */
  const triSolve = (upper, name, T, Y) => {
    T = asarray(T); Y = asarray(Y);
    const tn = upper ? 'U' : 'L';
    if (T.ndim < 2) throw new Error(`${name}(${tn},Y): ${tn}.ndim must be at least 2.`);
    if (Y.ndim < 2) throw new Error(`${name}(${tn},Y): Y.ndim must be at least 2.`);
    const M = Y.shape[Y.ndim - 2], J = Y.shape[Y.ndim - 1];
    if (T.shape[T.ndim - 2] !== M) throw new Error(`${name}(${tn},Y): ${tn} and Y don't match.`);
    if (T.shape[T.ndim - 1] !== M) throw new Error(`${name}(${tn},Y): Last two dimensions of ${tn} must be quadratic.`);
    if (!gpuOk(T) || !gpuOk(Y)) { if (fallback && fallback[name]) return fallback[name](T, Y); throw new Error(`nd4hip.${name}: dtype is not accelerated.`); }
    const lead = bcastLead([Array.from(T.shape.subarray(0, T.ndim - 2)), Array.from(Y.shape.subarray(0, Y.ndim - 2))], `${name}(${tn},Y): ${tn} and Y not broadcast-compatible.`);
    const dev = isDev(T) || isDev(Y), temps = [];
    const Td = opF64(T, dev, temps), Yd = opF64(Y, dev, temps), X = alloc(dev, lead.reduce((a, b) => a * b, 1) * M * J);
    for (const [cnt, [oT, oY], [sT, sY], b0] of bcastGroupsN(lead, [T.shape.subarray(0, T.ndim - 2), Y.shape.subarray(0, Y.ndim - 2)], [M * M, M * J]))
      native().dtrsm_batched(upper ? 1 : 0, 0, cnt, M, J, view(Td, oT), sT, view(Yd, oY), sY, view(X, b0 * M * J));
    release(temps);
    return wrap(dev, [...lead, M, J], X);
  };
  la.tril_solve = (L, Y) => triSolve(false, 'tril_solve', L, Y);
  la.triu_solve = (U, Y) => triSolve(true, 'triu_solve', U, Y);

  la.lu_solve = function lu_solve(LU, P, y) {
    if (undefined == y) { y = P; [LU, P] = LU; }
    LU = asarray(LU); if (LU.ndim < 2) throw new Error('LU must be at least 2D.');
    P = asarray(P); if (P.ndim < 1) throw new Error('P must be at least 1D.');
    y = asarray(y); if (y.ndim < 2) throw new Error('y must be at least 2D.');
    const N = LU.shape[LU.ndim - 2], I = y.shape[y.ndim - 2], J = y.shape[y.ndim - 1];
    if (LU.shape[LU.ndim - 1] != N) throw new Error('Last two dimensions of LU must be quadratic.');
    if (N != I) throw new Error("LU and y don't match.");
    if (N != P.shape[P.ndim - 1]) throw new Error("LU and P don't match.");
    if (!gpuOk(LU) || !gpuOk(y) || dtypeOf(P) !== 'int32') {
      if (fallback && fallback.lu_solve) return fallback.lu_solve(LU, P, y);
      throw new Error('nd4hip.lu_solve: dtype is not accelerated.');
    }
    const lLU = Array.from(LU.shape.subarray(0, LU.ndim - 2)), lP = Array.from(P.shape.subarray(0, P.ndim - 1)), lY = Array.from(y.shape.subarray(0, y.ndim - 2));
    let lead = bcastLead([lLU, lY], 'LU and y are not broadcast-compatible.');
    lead = bcastLead([lead, lP], 'P is not broadcast-compatible.');
    const dev = isDev(LU) || isDev(P) || isDev(y), temps = [];
    const X = alloc(dev, lead.reduce((a, b) => a * b, 1) * N * J), LUd = opF64(LU, dev, temps), Pd = opI32(P, dev, temps), yd = opF64(y, dev, temps);
    for (const [cnt, [oLU, oP, oY], [sLU, sP, sY], b0] of bcastGroupsN(lead, [lLU, lP, lY], [N * N, N, N * J]))
      native().dgetrs_batched(cnt, N, J, view(LUd, oLU), sLU, view(Pd, oP), sP, view(yd, oY), sY, view(X, b0 * N * J));
    release(temps);
    return wrap(dev, [...lead, N, J], X);
  };

  /* ---- SURVEY §8f N4: Cholesky (csrc/chol.hip) ---- */
  la.cholesky_decomp = function cholesky_decomp(S) {       // cholesky.js:51-71
    S = asarray(S);
    const nd_ = S.ndim;
    if (nd_ < 2 || S.shape[nd_ - 2] != S.shape[nd_ - 1]) throw new Error('Last two dimensions must be quadratic.');
    if (!gpuOk(S)) { if (fallback && fallback.cholesky_decomp) return fallback.cholesky_decomp(S); throw new Error('nd4hip.cholesky_decomp: dtype ' + dtypeOf(S) + ' is not accelerated.'); }
    const N = S.shape[nd_ - 1], batch = prod(S.shape, 0, nd_ - 2), dev = isDev(S), temps = [];
    const L = alloc(dev, batch * N * N);
    try { native().dpotrf_batched(batch, N, view(opF64(S, dev, temps), 0), view(L, 0)); }
    catch (e) { if (dev) L.free(); if (/near\) singular/.test(e.message)) throw new Error('Matrix contains NaNs or is (near) singular.'); throw e; }
    finally { release(temps); }
    return wrap(dev, S.shape, L);
  };

  la.cholesky_solve = function cholesky_solve(L, y) {      // cholesky.js:74-150
    L = asarray(L); y = asarray(y);
    if (L.ndim < 2) throw new Error('L must be at least 2D.');
    if (y.ndim < 2) throw new Error('y must be at least 2D.');
    const N = L.shape[L.ndim - 2], M = L.shape[L.ndim - 1], I = y.shape[y.ndim - 2], J = y.shape[y.ndim - 1];
    if (N != M) throw new Error('Last two dimensions of L must be quadratic.');
    if (I != M) throw new Error("L and y don't match.");
    if (!gpuOk(L) || !gpuOk(y)) { if (fallback && fallback.cholesky_solve) return fallback.cholesky_solve(L, y); throw new Error('nd4hip.cholesky_solve: dtype is not accelerated.'); }
    const lL = Array.from(L.shape.subarray(0, L.ndim - 2)), lY = Array.from(y.shape.subarray(0, y.ndim - 2));
    const lead = bcastLead([lL, lY], 'Shapes are not broadcast-compatible.');
    const dev = isDev(L) || isDev(y), temps = [];
    const X = alloc(dev, lead.reduce((a, b) => a * b, 1) * N * J), Ld = opF64(L, dev, temps), yd = opF64(y, dev, temps);
    for (const [cnt, [oL, oY], [sL, sY], b0] of bcastGroupsN(lead, [lL, lY], [N * N, N * J]))
      native().dpotrs_batched(cnt, N, J, view(Ld, oL), sL, view(yd, oY), sY, view(X, b0 * N * J));
    release(temps);
    return wrap(dev, [...lead, N, J], X);
  };

  la.ldl_decomp = function ldl_decomp(S) {                 // ldl.js:67-90
    S = asarray(S);
    const nd_ = S.ndim;
    if (nd_ < 2 || S.shape[nd_ - 2] !== S.shape[nd_ - 1]) throw new Error('Last two dimensions must be quadratic.');
    if (!gpuOk(S)) { if (fallback && fallback.ldl_decomp) return fallback.ldl_decomp(S); throw new Error('nd4hip.ldl_decomp: dtype ' + dtypeOf(S) + ' is not accelerated.'); }
    const N = S.shape[nd_ - 1], batch = prod(S.shape, 0, nd_ - 2), dev = isDev(S), temps = [];
    const LD = alloc(dev, batch * N * N);
    native().dldltrf_batched(batch, N, view(opF64(S, dev, temps), 0), view(LD, 0));
    release(temps);
    return wrap(dev, S.shape, LD);
  };

  la.ldl_solve = function ldl_solve(LD, y) {               // ldl.js:133-201
    LD = asarray(LD); y = asarray(y);
    if (LD.ndim < 2) throw new Error('ldl_solve(LD,y): LD must be at least 2D.');
    if (y.ndim < 2) throw new Error('ldl_solve(LD,y): y must be at least 2D.');
    const N = LD.shape[LD.ndim - 2], M = LD.shape[LD.ndim - 1], I = y.shape[y.ndim - 2], J = y.shape[y.ndim - 1];
    if (N != M) throw new Error('ldl_solve(LD,y): Last two dimensions of LD must be quadratic.');
    if (I != M) throw new Error("ldl_solve(LD,y): LD and y don't match.");
    if (!gpuOk(LD) || !gpuOk(y)) { if (fallback && fallback.ldl_solve) return fallback.ldl_solve(LD, y); throw new Error('nd4hip.ldl_solve: dtype is not accelerated.'); }
    const lL = Array.from(LD.shape.subarray(0, LD.ndim - 2)), lY = Array.from(y.shape.subarray(0, y.ndim - 2));
    const lead = bcastLead([lL, lY], 'Shapes are not broadcast-compatible.');
    const dev = isDev(LD) || isDev(y), temps = [];
    const X = alloc(dev, lead.reduce((a, b) => a * b, 1) * N * J), Ld = opF64(LD, dev, temps), yd = opF64(y, dev, temps);
    for (const [cnt, [oL, oY], [sL, sY], b0] of bcastGroupsN(lead, [lL, lY], [N * N, N * J]))
      native().dldltrs_batched(cnt, N, J, view(Ld, oL), sL, view(yd, oY), sY, view(X, b0 * N * J));
    release(temps);
    return wrap(dev, [...lead, N, J], X);
  };

  /* ---- pivoted LDL^T, Bunch-Kaufman (pldlp.js), csrc/pldlp.hip: LD and P are the reference's bits ---- */
  const PLDLP_TIERS = {auto: 0, lds: 1, global: 2, grid: 3};
  la.pldlp_decomp = function pldlp_decomp(S, opts) {       // pldlp.js:191-222; opts.tier (not in the reference): auto | lds | global | grid
    S = asarray(S);
    const nd_ = S.ndim;
    if (nd_ < 2 || S.shape[nd_ - 2] !== S.shape[nd_ - 1]) throw new Error('Last two dimensions must be quadratic.');
    const tier = opts && opts.tier != undefined ? PLDLP_TIERS[opts.tier] : 0;
    if (tier === undefined) throw new Error('pldlp_decomp(S): unknown tier ' + opts.tier + ' (auto, lds, global or grid).');
    if (!gpuOk(S)) { if (fallback && fallback.pldlp_decomp) return fallback.pldlp_decomp(S); throw new Error('nd4hip.pldlp_decomp: dtype ' + dtypeOf(S) + ' is not accelerated.'); }
    const N = S.shape[nd_ - 1], batch = prod(S.shape, 0, nd_ - 2), dev = isDev(S), temps = [];
    const LD = alloc(dev, batch * N * N), P = alloc(dev, batch * N, Int32Array);
    try { native().dsytrf_bk_batched(batch, N, view(opF64(S, dev, temps), 0), view(LD, 0), view(P, 0), tier); }
    catch (e) { if (dev) { LD.free(); P.free(); } throw e; }
    finally { release(temps); }
    return [wrap(dev, S.shape, LD), wrap(dev, S.shape.subarray(0, nd_ - 1), P)];
  };
  // the argument checks shared by pldlp_l / _d / _p (pldlp.js:231-236) and pldlp_solve (:529-537)
  const pldlpArgs = (LD, P, y) => {
    LD = asarray(LD); P = asarray(P);
    if (y !== undefined) y = asarray(y);
    if (LD.ndim < 2) throw new Error('pldlp_solve(LD,P,y): LD must be at least 2D.');
    if (P.ndim < 1) throw new Error('pldlp_solve(LD,P,y): P must be at least 1D.');
    if (y !== undefined && y.ndim < 2) throw new Error('pldlp_solve(LD,P,y): y must be at least 2D.');
    const N = LD.shape[LD.ndim - 2];
    if (N !== LD.shape[LD.ndim - 1]) throw new Error('pldlp_solve(LD,P,y): LD must be square.');
    if (N !== P.shape[P.ndim - 1]) throw new Error('pldlp_solve(LD,P,y): LD and P shape mismatch.');
    if (y !== undefined && N !== y.shape[y.ndim - 2]) throw new Error('pldlp_solve(LD,P,y): LD and y shape mismatch.');
    return [LD, P, y, N];
  };
  // P with the marks of the 2x2 blocks removed, after the complete check of pldlp.js:408-435 (last matrix and last row first)
  const pldlpPerm = (P, N) => {
    const p = P.data, out = new Int32Array(p.length), seen = new Uint8Array(N);
    for (let off = p.length - N; N > 0 && off >= 0; off -= N) {
      seen.fill(0);
      for (let i = N - 1; i >= 0; i--) {
        let q = p[off + i];
        if (q < 0) {
          if (i === 0 || p[off + i - 1] < 0) throw new Error('pldlp_solve(LD,P,y): P is invalid.');
          q = ~q;
        }
        if (!(q >= 0 && q < N)) throw new Error('pldlp_solve(LD,P,y): P contains out-of-bounds indices.');
        if (seen[q]) throw new Error('pldlp_solve(LD,P,y): P contains duplicate indices.');
        seen[q] = 1; out[off + i] = q;
      }
    }
    return out;
  };
  // pldlp_l / pldlp_d: host side, one N x N result per broadcast member of (LD, P)
  const pldlpFactor = (LD, P, member) => {
    if (P == undefined) [LD, P] = LD;
    let N; [LD, P, , N] = pldlpArgs(LD, P);
    const lL = Array.from(LD.shape.subarray(0, LD.ndim - 2)), lP = Array.from(P.shape.subarray(0, P.ndim - 1));
    const lead = bcastLead([lL, lP], 'Shapes are not broadcast-compatible.');
    const out = new Float64Array(lead.reduce((a, b) => a * b, 1) * N * N), ld = LD.data, p = P.data;
    for (const [cnt, [oL, oP], [sL, sP], b0] of bcastGroupsN(lead, [lL, lP], [N * N, N]))
      for (let c = 0; c < cnt; c++) member(N, ld, oL + c * sL, p, oP + c * sP, out, (b0 + c) * N * N);
    return new NDA(Int32Array.from([...lead, N, N]), out);
  };
  la.pldlp_l = (LD, P) => pldlpFactor(LD, P, (N, ld, oL, p, oP, out, o) => {           // pldlp.js:225-304
    for (let i = 0; i < N; i++) {
      const end = p[oP + i] < 0 ? i - 1 : i;             // the entry inside a 2x2 block belongs to D
      for (let j = 0; j < end; j++) out[o + N * i + j] = ld[oL + N * i + j];
      out[o + N * i + i] = 1;
    }
  });
  la.pldlp_d = (LD, P) => pldlpFactor(LD, P, (N, ld, oL, p, oP, out, o) => {           // pldlp.js:307-380
    for (let i = 0; i < N; i++) {
      out[o + N * i + i] = ld[oL + N * i + i];
      if (i > 0 && p[oP + i] < 0) out[o + N * i + i - 1] = out[o + N * (i - 1) + i] = ld[oL + N * i + i - 1];
    }
  });
  la.pldlp_p = function pldlp_p(LD, P) {                    // pldlp.js:383-438
    if (P == undefined) [LD, P] = LD;
    let N; [LD, P, , N] = pldlpArgs(LD, P);
    bcastLead([Array.from(LD.shape.subarray(0, LD.ndim - 2)), Array.from(P.shape.subarray(0, P.ndim - 1))], 'Shapes are not broadcast-compatible.');
    return new NDA(Int32Array.from(P.shape), pldlpPerm(P, N));
  };
  la.pldlp_solve = function pldlp_solve(LD, P, y) {         // pldlp.js:519-604
    if (y == undefined) {
      if (P == undefined) throw new Error('Assertion failed.');
      y = P; [LD, P] = LD;
    }
    let N; [LD, P, y, N] = pldlpArgs(LD, P, y);
    const J = y.shape[y.ndim - 1];
    if (!gpuOk(LD) || !gpuOk(y) || dtypeOf(P) !== 'int32') {
      if (fallback && fallback.pldlp_solve) return fallback.pldlp_solve(LD, P, y);
      throw new Error('nd4hip.pldlp_solve: dtype is not accelerated.');
    }
    const lL = Array.from(LD.shape.subarray(0, LD.ndim - 2)), lP = Array.from(P.shape.subarray(0, P.ndim - 1)), lY = Array.from(y.shape.subarray(0, y.ndim - 2));
    const lead = bcastLead([lL, lP, lY], 'Shapes are not broadcast-compatible.');
    pldlpPerm(P, N);                                        // P is checked completely on the host before any device work
    const dev = isDev(LD) || isDev(P) || isDev(y), temps = [];
    const X = alloc(dev, lead.reduce((a, b) => a * b, 1) * N * J), Ld = opF64(LD, dev, temps), Pd = opI32(P, dev, temps), yd = opF64(y, dev, temps);
    try {
      for (const [cnt, [oL, oP, oY], [sL, sP, sY], b0] of bcastGroupsN(lead, [lL, lP, lY], [N * N, N, N * J]))
        native().dsytrs_bk_batched(cnt, N, J, view(Ld, oL), sL, view(Pd, oP), sP, view(yd, oY), sY, view(X, b0 * N * J));
    } finally { release(temps); }
    return wrap(dev, [...lead, N, J], X);
  };

  la.bidiag_decomp = function bidiag_decomp(A) {           // bidiag.js:245-319
    A = asarray(A);
    if (A.ndim < 2) throw new Error('bidiag_decomp(A): A must be at least 2D.');
    if (String(dtypeOf(A)).startsWith('complex')) throw new Error('bidiag_decomp(A): complex A not yet supported.');
    if (!gpuOk(A)) { if (fallback && fallback.bidiag_decomp) return fallback.bidiag_decomp(A); throw new Error('nd4hip.bidiag_decomp: dtype ' + dtypeOf(A) + ' is not accelerated.'); }
    const nd_ = A.ndim, M = A.shape[nd_ - 2], N = A.shape[nd_ - 1], I = Math.min(M, N), J = M >= N ? I : I + 1, batch = prod(A.shape, 0, nd_ - 2);
    const Us = Int32Array.from(A.shape), Bs = Int32Array.from(A.shape), Vs = Int32Array.from(A.shape);
    Us[nd_ - 1] = I; Bs[nd_ - 2] = I; Bs[nd_ - 1] = J; Vs[nd_ - 2] = J;
    const dev = isDev(A), temps = [];
    const U = alloc(dev, batch * M * I), B = alloc(dev, batch * I * J), V = alloc(dev, batch * J * N);
    native().dgebrd_batched(batch, M, N, view(opF64(A, dev, temps), 0), view(U, 0), view(B, 0), view(V, 0));
    release(temps);
    return [wrap(dev, Us, U), wrap(dev, Bs, B), wrap(dev, Vs, V)];
  };

  la.hessenberg_decomp = function hessenberg_decomp(A) {   // hessenberg.js:89-115
    A = asarray(A);
    if (A.ndim < 2) throw new Error('hessenberg_decomp(A): A must at least be 2D.');
    const nd_ = A.ndim, N = A.shape[nd_ - 1];
    if (N != A.shape[nd_ - 2]) throw new Error('hessenberg_decomp(A): A must be square.');
    if (!gpuOk(A)) { if (fallback && fallback.hessenberg_decomp) return fallback.hessenberg_decomp(A); throw new Error('nd4hip.hessenberg_decomp: dtype ' + dtypeOf(A) + ' is not accelerated.'); }
    const batch = prod(A.shape, 0, nd_ - 2), dev = isDev(A), temps = [];
    const U = alloc(dev, batch * N * N), H = alloc(dev, batch * N * N);
    native().dgehrd_batched(batch, N, view(opF64(A, dev, temps), 0), view(U, 0), view(H, 0));
    release(temps);
    return [wrap(dev, A.shape, U), wrap(dev, A.shape, H)];
  };

  /* ---- least squares from a factorisation: qr_lstsq (qr.js:186-273), svd_lstsq / svd_solve (svd.js:66-228) ---- */
  la.qr_lstsq = function qr_lstsq(Q, R, y) {
    if (undefined == y) { y = R; [Q, R] = Q; }
    Q = asarray(Q); if (Q.ndim < 2) throw new Error('qr_lstsq(Q,R,y): Q.ndim must be at least 2.');
    R = asarray(R); if (R.ndim < 2) throw new Error('qr_lstsq(Q,R,y): R.ndim must be at least 2.');
    y = asarray(y); if (y.ndim < 2) throw new Error('qr_lstsq(Q,R,y): y.ndim must be at least 2.');
    const N = Q.shape[Q.ndim - 2], M = Q.shape[Q.ndim - 1], I = R.shape[R.ndim - 1], J = y.shape[y.ndim - 1];
    if (N != y.shape[y.ndim - 2]) throw new Error("qr_lstsq(Q,R,y): Q and y don't match.");
    if (M != R.shape[R.ndim - 2]) throw new Error("qr_lstsq(Q,R,y): Q and R don't match.");
    if (I > N) throw new Error('qr_lstsq(Q,R,y): Under-determined systems not supported. Use rrqr instead.');
    if (!gpuOk(Q) || !gpuOk(R) || !gpuOk(y)) {
      if (fallback && fallback.qr_lstsq) return fallback.qr_lstsq(Q, R, y);
      throw new Error('nd4hip.qr_lstsq: dtype is not accelerated.');
    }
    const lQ = Array.from(Q.shape.subarray(0, Q.ndim - 2)), lR = Array.from(R.shape.subarray(0, R.ndim - 2)), lY = Array.from(y.shape.subarray(0, y.ndim - 2));
    const lead = bcastLead([lQ, lR, lY], 'Q, R, y are not broadcast-compatible.');
    const dev = isDev(Q) || isDev(R) || isDev(y), temps = [];
    const X = alloc(dev, lead.reduce((a, b) => a * b, 1) * I * J), Qd = opF64(Q, dev, temps), Rd = opF64(R, dev, temps), yd = opF64(y, dev, temps);
    for (const [cnt, [oQ, oR, oY], [sQ, sR, sY], b0] of bcastGroupsN(lead, [lQ, lR, lY], [N * M, M * I, N * J]))
      native().dqrls_batched(cnt, N, M, I, J, view(Qd, oQ), sQ, view(Rd, oR), sR, view(yd, oY), sY, view(X, b0 * I * J));
    release(temps);
    return wrap(dev, [...lead, I, J], X);
  };

  la.svd_lstsq = function svd_lstsq(U, sv, V, y) {
    if (y == undefined) {
      if (V != undefined) throw new Error('svd_lstsq(Q,R,P, y): Either 2 ([Q,R,P], y) or 4 arguments (Q,R,P, y) expected.');
      y = sv; [U, sv, V] = U;
    }
    U = asarray(U); if (U.ndim < 2) throw new Error('svd_lstsq(U,sv,V, y): U.ndim must be at least 2.');
    sv = asarray(sv); if (sv.ndim < 1) throw new Error('svd_lstsq(U,sv,V, y): sv.ndim must be at least 1.');
    V = asarray(V); if (V.ndim < 2) throw new Error('svd_lstsq(U,sv,V, y): V.ndim must be at least 2.');
    y = asarray(y); if (y.ndim < 2) throw new Error('svd_lstsq(U,sv,V, y): y.ndim must be at least 2.');
    const N = U.shape[U.ndim - 2], M = U.shape[U.ndim - 1], I = V.shape[V.ndim - 1], J = y.shape[y.ndim - 1];
    if (N !== y.shape[y.ndim - 2]) throw new Error("svd_lstsq(U,sv,V, y): U and y don't match.");
    if (M !== sv.shape[sv.ndim - 1]) throw new Error("svd_lstsq(U,sv,V, y): U and sv don't match.");
    if (M !== V.shape[V.ndim - 2]) throw new Error("svd_lstsq(U,sv,V, y): V and sv don't match.");
    if (!gpuOk(U) || !gpuOk(sv) || !gpuOk(V) || !gpuOk(y)) {
      if (fallback && fallback.svd_lstsq) return fallback.svd_lstsq(U, sv, V, y);
      throw new Error('nd4hip.svd_lstsq: dtype is not accelerated.');
    }
    const lU = Array.from(U.shape.subarray(0, U.ndim - 2)), lS = Array.from(sv.shape.subarray(0, sv.ndim - 1)),
          lV = Array.from(V.shape.subarray(0, V.ndim - 2)), lY = Array.from(y.shape.subarray(0, y.ndim - 2));
    const lead = bcastLead([lU, lV, lY, lS], 'svd_lstsq(U,sv,V, y): U,sv,V,y not broadcast-compatible.');
    const svh = sv.data;                                     // tiny (batch x M): a device sv is read back once and cached
    for (let i = 0; i < svh.length; i++) if (!isFinite(svh[i])) throw new Error('svd_solve(): NaN or Infinity encountered.');   // svd.js:171-172
    const dev = isDev(U) || isDev(sv) || isDev(V) || isDev(y), temps = [];
    const X = alloc(dev, lead.reduce((a, b) => a * b, 1) * I * J), Ud = opF64(U, dev, temps), svd = opF64(sv, dev, temps), Vd = opF64(V, dev, temps), yd = opF64(y, dev, temps);
    for (const [cnt, [oU, oS, oV, oY], [sU, sS, sV, sY], b0] of bcastGroupsN(lead, [lU, lS, lV, lY], [N * M, M, M * I, N * J]))
      native().dsvdls_batched(cnt, N, M, I, J, view(Ud, oU), sU, view(svd, oS), sS, view(Vd, oV), sV, view(yd, oY), sY, view(X, b0 * I * J));
    release(temps);
    return wrap(dev, [...lead, I, J], X);
  };

  /* svd.js:66-97: the reference's singularity loop (`for( let r; r < N; r++ )`, :85) never executes, so apart from the
     squareness check svd_solve IS svd_lstsq; mirrored as such. */
  la.svd_solve = function svd_solve(U, sv, V, y) {
    if (y == undefined) {
      if (V != undefined) throw new Error('svd_lstsq(Q,R,P, y): Either 2 ([Q,R,P], y) or 4 arguments (Q,R,P, y) expected.');
      y = sv; [U, sv, V] = U;
    }
    U = asarray(U); sv = asarray(sv); V = asarray(V);
    if (U.shape[U.ndim - 2] !== V.shape[V.ndim - 1]) throw new Error('rrqr_solve(Q,R,P, y): System not square.');
    return la.svd_lstsq(U, sv, V, y);
  };
  /* svd.js:31-63: per matrix the first r with |sv_r| <= sqrt(eps) |sv_0| (entries are only examined up to that point, so a
     NaN behind the cut does not raise, exactly like the reference's loop). Host side: sv is tiny; a device array is read back. */
  la.svd_rank = function svd_rank(sv) {
    sv = la.to_host(asarray(sv));
    const N = sv.shape[sv.ndim - 1], data = sv.data, count = N > 0 ? data.length / N : 0, r = new Int32Array(count);
    const EPS = Math.sqrt(dtypeOf(sv) === 'float32' ? 2 ** -23 : 2 ** -52);
    for (let off = 0; off < count; off++) {
      const T = EPS * Math.abs(data[N * off]);
      for (; r[off] < N; r[off]++) {
        const x = Math.abs(data[N * off + r[off]]);
        if (!isFinite(x)) throw new Error('svd_rank(): NaN or Infinity encountered.');
        if (x <= T) break;
      }
    }
    return new NDA(Int32Array.from(sv.shape.subarray(0, sv.ndim - 1)), r);
  };

  /* ---- column-pivoted QR (rrqr.js) and solve (solve.js:23-27), csrc/rrqr.hip ---- */
  const rrqr = (name, full) => function (A) {
    A = asarray(A);
    if (A.ndim < 2) throw new Error('A must be at least 2D.');                     // rrqr.js:91 / :281
    if (!gpuOk(A)) { if (fallback && fallback[name]) return fallback[name](A); throw new Error('nd4hip.' + name + ': dtype ' + dtypeOf(A) + ' is not accelerated.'); }
    const nd_ = A.ndim, M = A.shape[nd_ - 2], N = A.shape[nd_ - 1], L = full ? M : Math.min(M, N), batch = prod(A.shape, 0, nd_ - 2);
    const lead = Array.from(A.shape.subarray(0, nd_ - 2));
    const dev = isDev(A), temps = [];
    const Q = alloc(dev, batch * M * L), R = alloc(dev, batch * L * N), P = alloc(dev, batch * N, Int32Array);
    native()[full ? 'dgeqp3_full_batched' : 'dgeqp3_batched'](batch, M, N, view(opF64(A, dev, temps), 0), view(Q, 0), view(R, 0), view(P, 0));
    release(temps);
    return [wrap(dev, [...lead, M, L], Q), wrap(dev, [...lead, L, N], R), wrap(dev, [...lead, N], P)];
  };
  la.rrqr_decomp = rrqr('rrqr_decomp', false);
  la.rrqr_decomp_full = rrqr('rrqr_decomp_full', true);
  const RANK_NAN = 'Infinity or NaN encountered during rank estimation.';
  const hostInts = x => x instanceof DevBuf ? new DeviceNDArray(Int32Array.of(x.length), x).data : x;
  la.rrqr_rank = function rrqr_rank(R) {                     // rrqr.js:398-414
    R = asarray(R);
    if (R.ndim < 2) throw new Error('rrqr_rank(R): R.ndim must be at least 2.');
    if (!gpuOk(R)) { if (fallback && fallback.rrqr_rank) return fallback.rrqr_rank(R); throw new Error('nd4hip.rrqr_rank: dtype ' + dtypeOf(R) + ' is not accelerated.'); }
    const nd_ = R.ndim, M = R.shape[nd_ - 2], N = R.shape[nd_ - 1], batch = prod(R.shape, 0, nd_ - 2);
    const dev = isDev(R), temps = [], r = alloc(dev, batch, Int32Array);
    native().dqp3rank_batched(batch, M, N, view(opF64(R, dev, temps), 0), view(r, 0));
    release(temps);
    if (dev && hostInts(r).some(k => k < 0)) throw new Error(RANK_NAN);             // the _dev form marks it with -1
    return wrap(dev, Array.from(R.shape.subarray(0, nd_ - 2)), r);
  };
  const rrqrArgs = (Q, R, P, y) => {
    if (y == undefined) {
      if (P != undefined) throw new Error('rrqr_lstsq(Q,R,P, y): Either 2 ([Q,R,P], y) or 4 arguments (Q,R,P, y) expected.');
      y = R; [Q, R, P] = Q;
    }
    return [Q, R, P, y];
  };
  // rrqr.js:447-580 -> [X, ranks (host Int32Array or device buffer)]; null when the dtypes are not accelerated
  const rrqrLstsq = (Q, R, P, y) => {
    Q = asarray(Q); if (Q.ndim < 2) throw new Error('rrqr_lstsq(Q,R,P, y): Q.ndim must be at least 2.');
    R = asarray(R); if (R.ndim < 2) throw new Error('rrqr_lstsq(Q,R,P, y): R.ndim must be at least 2.');
    P = asarray(P); if (P.ndim < 1) throw new Error('rrqr_lstsq(Q,R,P, y): P.ndim must be at least 1.');
    y = asarray(y); if (y.ndim < 2) throw new Error('rrqr_lstsq(Q,R,P, y): y.ndim must be at least 2.');
    if (dtypeOf(P) !== 'int32') throw new Error('rrqr_lstsq(Q,R,P, y): P.dtype must be "int32".');
    const N = Q.shape[Q.ndim - 2], M = Q.shape[Q.ndim - 1], I = R.shape[R.ndim - 1], J = y.shape[y.ndim - 1];
    if (N != y.shape[y.ndim - 2]) throw new Error("rrqr_lstsq(Q,R,P,y): Q and y don't match.");
    if (M != R.shape[R.ndim - 2]) throw new Error("rrqr_lstsq(Q,R,P,y): Q and R don't match.");
    if (I != P.shape[P.ndim - 1]) throw new Error("rrqr_lstsq(Q,R,P,y): R and P don't match.");
    const lQ = Array.from(Q.shape.subarray(0, Q.ndim - 2)), lR = Array.from(R.shape.subarray(0, R.ndim - 2)),
          lP = Array.from(P.shape.subarray(0, P.ndim - 1)), lY = Array.from(y.shape.subarray(0, y.ndim - 2));
    const lead = bcastLead([lQ, lR, lY, lP], 'rrqr_lstsq(Q,R,P,y): Q,R,P,y not broadcast-compatible.');
    if (!gpuOk(Q) || !gpuOk(R) || !gpuOk(y)) return null;
    const total = lead.reduce((a, b) => a * b, 1);
    const dev = isDev(Q) || isDev(R) || isDev(P) || isDev(y), temps = [];
    const X = alloc(dev, total * I * J), ranks = alloc(dev, total, Int32Array);
    const Qd = opF64(Q, dev, temps), Rd = opF64(R, dev, temps), Pd = opI32(P, dev, temps), yd = opF64(y, dev, temps);
    try {
      for (const [cnt, [oQ, oR, oP, oY], [sQ, sR, sP, sY], b0] of bcastGroupsN(lead, [lQ, lR, lP, lY], [N * M, M * I, I, N * J]))
        native().dqp3ls_batched(cnt, N, M, I, J, view(Qd, oQ), sQ, view(Rd, oR), sR, view(Pd, oP), sP, view(yd, oY), sY,
                                view(X, b0 * I * J), view(ranks, b0));
    } finally { release(temps); }
    if (dev && hostInts(ranks).some(k => k < 0)) throw new Error(RANK_NAN);
    return [wrap(dev, [...lead, I, J], X), ranks];
  };
  la.rrqr_lstsq = function rrqr_lstsq(Q, R, P, y) {
    [Q, R, P, y] = rrqrArgs(Q, R, P, y);
    const out = rrqrLstsq(Q, R, P, y);
    if (out) return out[0];
    if (fallback && fallback.rrqr_lstsq) return fallback.rrqr_lstsq(Q, R, P, y);
    throw new Error('nd4hip.rrqr_lstsq: dtype is not accelerated.');
  };
  la.rrqr_solve = function rrqr_solve(Q, R, P, y) {          // rrqr.js:417-444
    [Q, R, P, y] = rrqrArgs(Q, R, P, y);
    Q = asarray(Q); R = asarray(R);
    const N = Q.shape[Q.ndim - 2];
    if (N !== R.shape[R.ndim - 1]) throw new Error('rrqr_solve(Q,R,P, y): Q @ R not square.');
    const out = rrqrLstsq(Q, R, P, y);
    if (!out) {
      if (fallback && fallback.rrqr_solve) return fallback.rrqr_solve(Q, R, P, y);
      throw new Error('nd4hip.rrqr_solve: dtype is not accelerated.');
    }
    const [x, ranks] = out;
    if (hostInts(ranks).some(k => k < N)) throw new SolveError(la.to_host(x));
    return x;
  };
  la.solve = function solve(A, y) {                            // solve.js:23-27
    const [Q, R, P] = la.rrqr_decomp(A);
    return la.rrqr_solve(Q, R, P, y);
  };
  la.SingularMatrixSolveError = SolveError;

  /* ---- strong rank-revealing QR (srrqr.js) and URV (urv.js), csrc/srrqr.hip ---- */
  const jsNum = x => Number.isNaN(x) ? 'NaN' : String(x);
  const isArr = x => x instanceof NDA || !!(x && x.shape && x.data);
  la.srrqr_decomp_full = function srrqr_decomp_full(A, opt = {}) {
    A = asarray(A);
    if (A.ndim < 2) throw new Error('srrqr_decomp_full(A,opt): A must be at least 2D.');
    const {dtol = 1.01, ztol = undefined} = opt || {};
    if (isArr(dtol)) throw new Error('srrqr_decomp_full(A,opt): NDArray as opt.dtol not yet supported.');
    if (!(dtol >= 1)) throw new Error(`srrqr_decomp_full(A,opt): Invalid opt.dtol: ${jsNum(dtol)}. Must be >=1.`);
    if (isArr(ztol)) throw new Error('srrqr_decomp_full(A,opt): NDArray as opt.ztol not yet supported.');
    if (ztol != null && !(ztol >= 0)) throw new Error(`srrqr_decomp_full(A,opt): invalid opt.ztol: ${jsNum(ztol)}. Must be non-negative number.`);
    if (!gpuOk(A)) { if (fallback && fallback.srrqr_decomp_full) return fallback.srrqr_decomp_full(A, opt); throw new Error('nd4hip.srrqr_decomp_full: dtype ' + dtypeOf(A) + ' is not accelerated.'); }
    if (!isFinite(dtol)) throw new Error(`Assertion failed. Invalid dtol: ${dtol}.`);
    if (ztol != null && !isFinite(ztol)) throw new Error(`Assertion failed. Invalid ztol: ${ztol}.`);
    const nd_ = A.ndim, M = A.shape[nd_ - 2], N = A.shape[nd_ - 1], batch = prod(A.shape, 0, nd_ - 2);
    const lead = Array.from(A.shape.subarray(0, nd_ - 2));
    const dev = isDev(A), temps = [];
    const Q = alloc(dev, batch * M * M), R = alloc(dev, batch * M * N), P = alloc(dev, batch * N, Int32Array), r = alloc(dev, batch, Int32Array);
    try {
      native().dsrrqr_batched(batch, M, N, view(opF64(A, dev, temps), 0), +dtol, ztol == null ? -1 : +ztol, view(Q, 0), view(R, 0), view(P, 0), view(r, 0));
    } finally { release(temps); }
    return [wrap(dev, [...lead, M, M], Q), wrap(dev, [...lead, M, N], R), wrap(dev, [...lead, N], P), wrap(dev, lead, r)];
  };
  la.urv_decomp_full = function urv_decomp_full(A) {           // urv.js:100-135
    A = asarray(A);
    if (A.ndim < 2) throw new Error('srrqr_decomp_full(A,opt): A must be at least 2D.');
    if (!gpuOk(A)) { if (fallback && fallback.urv_decomp_full) return fallback.urv_decomp_full(A); throw new Error('nd4hip.urv_decomp_full: dtype ' + dtypeOf(A) + ' is not accelerated.'); }
    const nd_ = A.ndim, M = A.shape[nd_ - 2], N = A.shape[nd_ - 1], batch = prod(A.shape, 0, nd_ - 2);
    const lead = Array.from(A.shape.subarray(0, nd_ - 2));
    const dev = isDev(A), temps = [];
    const U = alloc(dev, batch * M * M), R = alloc(dev, batch * M * N), V = alloc(dev, batch * N * N), r = alloc(dev, batch, Int32Array);
    try { native().durv_batched(batch, M, N, view(opF64(A, dev, temps), 0), view(U, 0), view(R, 0), view(V, 0), view(r, 0)); }
    finally { release(temps); }
    return [wrap(dev, [...lead, M, M], U), wrap(dev, [...lead, M, N], R), wrap(dev, [...lead, N, N], V), wrap(dev, lead, r)];
  };
  la.urv_lstsq = function urv_lstsq(U, R, V, ranks, Y) {        // urv.js:138-323
    if (Y == null) {
      if (ranks != null || V != null) throw new Error('urv_lstsq( U,R,V,ranks, Y ): Either 2 ([U,R,V,ranks], Y) or 5 arguments (U,R,V,ranks, Y) expected.');
      Y = R; [U, R, V, ranks] = U;
    }
    U = asarray(U); if (!(U.ndim >= 2)) throw new Error('urv_lstsq(U,R,V, Y): U.ndim must be at least 2.');
    R = asarray(R); if (!(R.ndim >= 2)) throw new Error('urv_lstsq(U,R,V, Y): R.ndim must be at least 2.');
    V = asarray(V); if (!(V.ndim >= 2)) throw new Error('urv_lstsq(U,R,V, Y): V.ndim must be at least 2.');
    Y = asarray(Y); if (!(Y.ndim >= 2)) throw new Error('urv_lstsq(U,R,V, Y): Y.ndim must be at least 2.');
    ranks = asarray(ranks);
    const lU = Array.from(U.shape.subarray(0, U.ndim - 2)), lR = Array.from(R.shape.subarray(0, R.ndim - 2)),
          lV = Array.from(V.shape.subarray(0, V.ndim - 2)), lY = Array.from(Y.shape.subarray(0, Y.ndim - 2)), lK = Array.from(ranks.shape);
    const lead = bcastLead([lU, lR, lV, lY, lK], 'urv_lstsq( U,R,V,ranks, Y ): U,R,V,ranks, Y not broadcast-compatible.');
    const I = U.shape[U.ndim - 2], J = U.shape[U.ndim - 1], K = V.shape[V.ndim - 2], L = V.shape[V.ndim - 1], Jc = Y.shape[Y.ndim - 1];
    if (R.shape[R.ndim - 2] !== J || R.shape[R.ndim - 1] !== K || Y.shape[Y.ndim - 2] !== I) throw new Error('urv_lstsq( U,R,V,ranks, Y ): Matrix dimensions incompatible.');
    if (J !== K && ((I < L && I !== J) || (I >= L && K !== L))) throw new Error('Assertion failed.');
    if (!(I >= J) || !(K <= L)) throw new Error('Assertion failed.');
    if (!gpuOk(U) || !gpuOk(R) || !gpuOk(V) || !gpuOk(Y)) {
      if (fallback && fallback.urv_lstsq) return fallback.urv_lstsq(U, R, V, ranks, Y);
      throw new Error('nd4hip.urv_lstsq: dtype is not accelerated.');
    }
    const total = lead.reduce((a, b) => a * b, 1);
    const dev = isDev(U) || isDev(R) || isDev(V) || isDev(Y) || isDev(ranks), temps = [];
    const X = alloc(dev, total * L * Jc);
    const Ud = opF64(U, dev, temps), Rd = opF64(R, dev, temps), Vd = opF64(V, dev, temps), Kd = opI32(ranks, dev, temps), Yd = opF64(Y, dev, temps);
    try {
      for (const [cnt, [oU, oR, oV, oK, oY], [sU, sR, sV, sK, sY], b0] of bcastGroupsN(lead, [lU, lR, lV, lK, lY], [I * J, J * K, K * L, 1, I * Jc]))
        native().durvls_batched(cnt, I, J, K, L, Jc, view(Ud, oU), sU, view(Rd, oR), sR, view(Vd, oV), sV, view(Kd, oK), sK, view(Yd, oY), sY,
                                view(X, b0 * L * Jc));
    } finally { release(temps); }
    return wrap(dev, [...lead, L, Jc], X);
  };

  /* ---- det / slogdet / det_tri / slogdet_tri (det.js), rank (rank.js), lstsq (lstsq.js), norm (norm.js), csrc/det.hip ---- */
  const f64Only = a => dtypeOf(a) === 'float64';
  const detCommon = (name, logForm, A) => {
    A = asarray(A);
    if (A.ndim < 2) throw new Error('qr_decomp(A): A.ndim must be at least 2.');                 // det.js:97 / :104: qr_decomp first
    if (!f64Only(A)) { if (fallback && fallback[name]) return fallback[name](A); throw new Error(`nd4hip.${name}: dtype ${dtypeOf(A)} is not accelerated.`); }
    const nd_ = A.ndim, M = A.shape[nd_ - 2], N = A.shape[nd_ - 1], batch = prod(A.shape, 0, nd_ - 2);
    if (M < N) throw new Error(logForm ? 'det_tri(A): A must be square matrices.' : 'det_tri(a): a must be square matrices.');
    const lead = Array.from(A.shape.subarray(0, nd_ - 2));
    const dev = isDev(A), temps = [];
    const D = alloc(dev, batch), L = logForm ? alloc(dev, batch) : null;
    try {
      if (logForm) native().dslogdet_batched(batch, M, N, view(opF64(A, dev, temps), 0), view(D, 0), view(L, 0));
      else native().ddet_batched(batch, M, N, view(opF64(A, dev, temps), 0), view(D, 0));
    } finally { release(temps); }
    return logForm ? [wrap(dev, lead, D), wrap(dev, lead, L)] : wrap(dev, lead, D);
  };
  la.det = function det(A) { return detCommon('det', false, A); };
  la.slogdet = function slogdet(A) { return detCommon('slogdet', true, A); };
  const detTriCommon = (name, logForm, A) => {
    A = asarray(A);
    if (A.ndim < 2) throw new Error(logForm ? 'det_tri(A): A.ndim must be at least 2.' : `det_tri(a): a.shape=[${Array.from(A.shape)}]; a.ndim must be at least 2.`);
    const nd_ = A.ndim, M = A.shape[nd_ - 2], N = A.shape[nd_ - 1], batch = prod(A.shape, 0, nd_ - 2);
    if (M !== N) throw new Error(logForm ? 'det_tri(A): A must be square matrices.' : 'det_tri(a): a must be square matrices.');
    if (!f64Only(A)) { if (fallback && fallback[name]) return fallback[name](A); throw new Error(`nd4hip.${name}: dtype ${dtypeOf(A)} is not accelerated.`); }
    const lead = Array.from(A.shape.subarray(0, nd_ - 2));
    const dev = isDev(A), temps = [];
    const D = alloc(dev, batch), L = logForm ? alloc(dev, batch) : null;
    try {
      if (logForm) native().dslogdettri_batched(batch, N, view(opF64(A, dev, temps), 0), view(D, 0), view(L, 0));
      else native().ddettri_batched(batch, N, view(opF64(A, dev, temps), 0), view(D, 0));
    } finally { release(temps); }
    return logForm ? [wrap(dev, lead, D), wrap(dev, lead, L)] : wrap(dev, lead, D);
  };
  la.det_tri = function det_tri(A) { return detTriCommon('det_tri', false, A); };
  la.slogdet_tri = function slogdet_tri(A) { return detTriCommon('slogdet_tri', true, A); };
  la.rank = function rank(A) {                                   // rank.js:23-27
    const [, sv] = la.svd_decomp(A);
    return la.svd_rank(sv);
  };
  la.lstsq = function lstsq(A, y) {                              // lstsq.js:22-26
    const [U, sv, V] = la.svd_decomp(A);
    return la.svd_lstsq(U, sv, V, y);
  };
  la.norm = function norm(A, ord = 'fro', axis = undefined) {    // norm.js:74-85: a number, also for a DeviceNDArray
    A = asarray(A);
    if (ord !== 'fro') throw new Error(`norm(A,ord,axis): Unsupported ord: ${ord}.`);
    if (axis != null) throw new Error('norm(A,ord,axis): axis argument not yet supported.');
    if (!f64Only(A)) { if (fallback && fallback.norm) return fallback.norm(A, ord, axis); throw new Error('nd4hip.norm: dtype ' + dtypeOf(A) + ' is not accelerated.'); }
    const n = prod(A.shape, 0, A.ndim);
    return native().dnrmfro(n, isDev(A) ? view(A._buf, 0) : A.data);
  };

  /* ---- schur_eigenvals / schur_eigen (schur.js:31-370), eigen_balance_pre / _post (eigen.js:91-270), csrc/eigvec.hip ---- */
  const wrapZ = (name, dev, shape, x) => { const Cx = needComplex(name);
    return dev ? new DeviceNDArray(Int32Array.from(shape), x, Cx) : new NDA(Int32Array.from(shape), complexOver(Cx, x)); };
  const evFallback = (name, args) => { if (fallback && fallback[name]) return fallback[name](...args); throw new Error(`nd4hip.${name}: dtype is not accelerated.`); };
  la.schur_eigenvals = function schur_eigenvals(T) {
    T = asarray(T);
    const nd_ = T.ndim, N = T.shape[nd_ - 1];
    if (nd_ < 2 || T.shape[nd_ - 2] !== N) throw new Error('T is not square.');
    if (!f64Only(T)) return evFallback('schur_eigenvals', [T]);
    const batch = prod(T.shape, 0, nd_ - 2), dev = isDev(T), temps = [];
    const L = alloc(dev, 2 * batch * N);
    try { native().dtreval_batched(batch, N, view(opF64(T, dev, temps), 0), view(L, 0)); } finally { release(temps); }
    return wrapZ('schur_eigenvals', dev, Array.from(T.shape.subarray(0, nd_ - 1)), L);
  };
  la.schur_eigen = function schur_eigen(Q, T) {
    Q = asarray(Q); T = asarray(T);
    if (Q.ndim !== T.ndim) throw new Error('Q.ndim != T.ndim.');
    for (let i = T.ndim; i-- > 0;) if (Q.shape[i] !== T.shape[i]) throw new Error('Q.shape != T.shape.');
    const nd_ = T.ndim, N = T.shape[nd_ - 1];
    if (nd_ < 2 || T.shape[nd_ - 2] !== N) throw new Error('Q is not square.');
    if (!f64Only(Q) || !f64Only(T)) return evFallback('schur_eigen', [Q, T]);
    const batch = prod(T.shape, 0, nd_ - 2), dev = isDev(Q) || isDev(T), temps = [];
    const L = alloc(dev, 2 * batch * N), V = alloc(dev, 2 * batch * N * N);
    try { native().dtrevc_batched(batch, N, view(opF64(Q, dev, temps), 0), view(opF64(T, dev, temps), 0), view(L, 0), view(V, 0)); } finally { release(temps); }
    return [wrapZ('schur_eigen', dev, Array.from(T.shape.subarray(0, nd_ - 1)), L), wrapZ('schur_eigen', dev, Array.from(T.shape), V)];
  };
  la.eigen_balance_pre = function eigen_balance_pre(A, p) {
    A = asarray(A);
    if (p == null) p = 2;
    if (!(p >= 1)) throw new Error(`Invalid norm p=${p};`);
    const nd_ = A.ndim, N = A.shape[nd_ - 1];
    if (nd_ < 2 || A.shape[nd_ - 2] !== N) throw new Error('A is not square');
    if (!f64Only(A)) return evFallback('eigen_balance_pre', [A, p]);
    const batch = prod(A.shape, 0, nd_ - 2), dev = isDev(A), temps = [];
    const D = alloc(dev, batch * N), B = alloc(dev, batch * N * N);
    try { native().dgebal_batched(batch, N, +p, view(opF64(A, dev, temps), 0), view(D, 0), view(B, 0)); } finally { release(temps); }
    return [wrap(dev, Array.from(A.shape.subarray(0, nd_ - 1)), D), wrap(dev, Array.from(A.shape), B)];
  };
  la.eigen_balance_post = function eigen_balance_post(D, V) {
    D = asarray(D); V = asarray(V);
    if (V.ndim < 2) throw new Error('eigen_balance_post(D,V): V.ndim must be at least 2.');
    const nd_ = V.ndim, N = V.shape[nd_ - 1];
    if (V.shape[nd_ - 2] !== N) throw new Error('eigen_balance_post(D,V): V must be square.');
    // the accelerated form takes a complex128 V and a float64 D of V's leading shape; anything else is the host module's
    let same = D.ndim === nd_ - 1;
    for (let i = 0; same && i < D.ndim; i++) same = D.shape[i] === V.shape[i];
    if (!same || !f64Only(D) || dtypeOf(V) !== 'complex128') return evFallback('eigen_balance_post', [D, V]);
    const batch = prod(V.shape, 0, nd_ - 2), dev = isDev(D) || isDev(V), temps = [];
    const W = alloc(dev, 2 * batch * N * N);
    try { native().zgebak_batched(batch, N, view(opF64(D, dev, temps), 0), view(opZ(V, dev, temps), 0), view(W, 0)); } finally { release(temps); }
    return wrapZ('eigen_balance_post', dev, Array.from(V.shape), W);
  };

  /* ---- schur_decomp (schur.js:372-683), eigen / eigenvals (eigen.js:33-88), csrc/schur.hip. The reference's eigen calls its
   * module-internal schur_decomp, so eigen and eigenvals are composed on the device (dgeev) and not from the patched names ---- */
  const squareOr = (A, ndimText, squareText) => {
    if (A.ndim < 2) throw new Error(ndimText);
    if (A.shape[A.ndim - 2] !== A.shape[A.ndim - 1]) throw new Error(squareText);
  };
  la.schur_decomp = function schur_decomp(A) {
    A = asarray(A);
    squareOr(A, 'hessenberg_decomp(A): A must at least be 2D.', 'hessenberg_decomp(A): A must be square.');
    if (!f64Only(A)) return evFallback('schur_decomp', [A]);
    const nd_ = A.ndim, N = A.shape[nd_ - 1], batch = prod(A.shape, 0, nd_ - 2), dev = isDev(A), temps = [];
    const Q = alloc(dev, batch * N * N), T = alloc(dev, batch * N * N);
    try { native().dgees_batched(batch, N, view(opF64(A, dev, temps), 0), view(Q, 0), view(T, 0)); } finally { release(temps); }
    return [wrap(dev, Array.from(A.shape), Q), wrap(dev, Array.from(A.shape), T)];
  };
  // the reference's private in-place step as a function of (U, H) returning new arrays: [Q, T]
  la.schur_qrfrancis = function schur_qrfrancis(U, H) {
    U = asarray(U); H = asarray(H);
    if (U.ndim < 2 || U.shape[U.ndim - 2] !== U.shape[U.ndim - 1]) throw new Error('Q is not square.');
    if (U.ndim !== H.ndim) throw new Error('Q.ndim != H.ndim.');
    for (let i = U.ndim; i-- > 0;) if (U.shape[i] !== H.shape[i]) throw new Error('Q.shape != H.shape.');
    if (!f64Only(U) || !f64Only(H)) throw new Error('nd4hip.schur_qrfrancis: dtype is not accelerated.');
    const nd_ = U.ndim, N = U.shape[nd_ - 1], batch = prod(U.shape, 0, nd_ - 2), dev = isDev(U) || isDev(H), temps = [];
    const Q = alloc(dev, batch * N * N), T = alloc(dev, batch * N * N);
    try { native().dhseqr_batched(batch, N, view(opF64(U, dev, temps), 0), view(opF64(H, dev, temps), 0), view(Q, 0), view(T, 0)); } finally { release(temps); }
    return [wrap(dev, Array.from(U.shape), Q), wrap(dev, Array.from(U.shape), T)];
  };
  la.eigen = function eigen(A) {
    A = asarray(A);
    squareOr(A, 'A is not square', 'A is not square');
    if (!f64Only(A)) return evFallback('eigen', [A]);
    needComplex('eigen');
    const nd_ = A.ndim, N = A.shape[nd_ - 1], batch = prod(A.shape, 0, nd_ - 2), dev = isDev(A), temps = [];
    const L = alloc(dev, 2 * batch * N), V = alloc(dev, 2 * batch * N * N);
    try { native().dgeev_batched(batch, N, view(opF64(A, dev, temps), 0), view(L, 0), view(V, 0)); } finally { release(temps); }
    return [wrapZ('eigen', dev, Array.from(A.shape.subarray(0, nd_ - 1)), L), wrapZ('eigen', dev, Array.from(A.shape), V)];
  };
  la.eigenvals = function eigenvals(A) {
    A = asarray(A);
    squareOr(A, 'A is not square', 'A is not square');
    if (!f64Only(A)) return evFallback('eigenvals', [A]);
    needComplex('eigenvals');
    const nd_ = A.ndim, N = A.shape[nd_ - 1], batch = prod(A.shape, 0, nd_ - 2), dev = isDev(A), temps = [];
    const L = alloc(dev, 2 * batch * N);
    try { native().dgeevals_batched(batch, N, view(opF64(A, dev, temps), 0), view(L, 0)); } finally { release(temps); }
    return wrapZ('eigenvals', dev, Array.from(A.shape.subarray(0, nd_ - 1)), L);
  };

  /* ---- structure functions: tril / triu (tri.js:23-42), diag / diag_mat (diag.js:23-88), permute_rows / permute_cols /
   * unpermute_rows / unpermute_cols (permute.js:23-306), csrc/struct.hip. Values are moved, never computed. ---- */
  // a device argument is never handed to the host module: its function would read `.data`, a silent download of the whole array
  const structFallback = (name, args) => { if (fallback && fallback[name] && !args.some(isDev)) return fallback[name](...args); throw new Error(`nd4hip.${name}: dtype is not accelerated.`); };
  // i < j - k is floor(k) < j - i and i > j - k is ceil(k) > j - i for integer i, j: any number k maps to an integer; NaN never cuts
  const MAXK = Math.pow(2, 53);
  const triK = (upper, k) => { k = +k; if (k !== k) return upper ? -MAXK : MAXK; return Math.max(-MAXK, Math.min(MAXK, upper ? Math.ceil(k) : Math.floor(k))); };
  const tri = (upper, name) => function (m, k = 0) {
    m = asarray(m);
    if (m.ndim < 2) throw new Error('Input must be at least 2D.');
    if (!f64Only(m)) return structFallback(name, [m, k]);
    const nd_ = m.ndim, M = m.shape[nd_ - 2], N = m.shape[nd_ - 1], batch = prod(m.shape, 0, nd_ - 2), dev = isDev(m), temps = [];
    const B = alloc(dev, batch * M * N);
    try { native().dtri_batched(upper, triK(upper, k), batch, M, N, view(opF64(m, dev, temps), 0), view(B, 0)); } finally { release(temps); }
    return wrap(dev, m.shape, B);
  };
  la.tril = tri(0, 'tril'); Object.defineProperty(la.tril, 'name', {value: 'tril'});
  la.triu = tri(1, 'triu'); Object.defineProperty(la.triu, 'name', {value: 'triu'});
  la.diag = function diag(A, offset = 0) {
    A = asarray(A);
    if (A.ndim < 2) throw new Error(`diag(A, offset): A.ndim=${A.ndim} is less than 2.`);
    const nd_ = A.ndim, M = A.shape[nd_ - 2], N = A.shape[nd_ - 1];
    if (!(offset > -M && offset < +N)) throw new Error(`diag(A, offset): offset=${offset} out of A.shape=[undefined].`);   // (the reference prints the shape of A.data)
    if (!f64Only(A) || !Number.isInteger(+offset)) return structFallback('diag', [A, offset]);
    const L = Math.min(M, M + offset, N, N - offset), batch = prod(A.shape, 0, nd_ - 2), dev = isDev(A), temps = [];
    const d = alloc(dev, batch * L);
    try { native().ddiag_batched(batch, M, N, +offset, view(opF64(A, dev, temps), 0), view(d, 0)); } finally { release(temps); }
    return wrap(dev, [...A.shape.subarray(0, nd_ - 2), L], d);
  };
  la.diag_mat = function diag_mat(diag) {
    diag = asarray(diag);
    if (diag.ndim < 1) throw new Error(`diag_mat(diag): diag.ndim=${diag.ndim} is less than 1.`);
    const N = diag.shape[diag.ndim - 1];
    if (N <= 0) throw new Error('Assertion Failed!');
    if (!f64Only(diag)) return structFallback('diag_mat', [diag]);
    const batch = prod(diag.shape, 0, diag.ndim - 1), dev = isDev(diag), temps = [];
    const D = alloc(dev, batch * N * N);
    try { native().ddiagmat_batched(batch, N, view(opF64(diag, dev, temps), 0), view(D, 0)); } finally { release(temps); }
    return wrap(dev, [...diag.shape, N], D);
  };
  const permute = (cols, inverse, name) => {
    const f = function (A, P) {
      A = asarray(A); if (A.ndim < 2) throw new Error(`${name}(A,P): A.ndim must be at least 2.`);
      P = asarray(P); if (P.ndim < 1) throw new Error(`${name}(A,P): P.ndim must be at least 1.`);
      if (!f64Only(A) || dtypeOf(P) !== 'int32') return structFallback(name, [A, P]);
      const M = A.shape[A.ndim - 2], N = A.shape[A.ndim - 1], L = cols ? N : M;
      if (L !== P.shape[P.ndim - 1]) throw new Error(`${name}(A,P): A.shape[${cols ? -1 : -2}] and P.shape[-1] must match.`);
      const lA = Array.from(A.shape.subarray(0, A.ndim - 2)), lP = Array.from(P.shape.subarray(0, P.ndim - 1));
      const lead = bcastLead([lA, lP], `${name}(A,P): A and P not broadcast-compatible.`);      // max(A.ndim, P.ndim + 1) axes in all
      const dev = isDev(A) || isDev(P), temps = [];
      const B = alloc(dev, lead.reduce((a, b) => a * b, 1) * M * N);
      try {
        const Ad = opF64(A, dev, temps), Pd = opI32(P, dev, temps);
        for (const [cnt, [oA, oP], [sA, sP], b0] of bcastGroupsN(lead, [lA, lP], [M * N, L]))
          native().dpermute_batched(cols, inverse, cnt, M, N, view(Ad, oA), sA, view(Pd, oP), sP, view(B, b0 * M * N));
      } finally { release(temps); }
      return wrap(dev, [...lead, M, N], B);
    };
    Object.defineProperty(f, 'name', {value: name});
    return f;
  };
  la.permute_rows = permute(0, 0, 'permute_rows');
  la.permute_cols = permute(1, 0, 'permute_cols');
  la.unpermute_rows = permute(0, 1, 'unpermute_rows');
  la.unpermute_cols = permute(1, 1, 'unpermute_cols');

  /* ---- concat (concat.js) / stack (stack.js) on device arrays, csrc/gather.hip: (axis?, dtype?, arrays) as the reference's nd.concat
   * and nd.stack. At least one array must be a DeviceNDArray; host arrays in the list are uploaded on the way in; all arrays share one
   * dtype (float64, int32 or complex128) and `dtype`, if given, names it: a conversion would compute, this only moves. Results are
   * DeviceNDArrays. Not enumerable, like to_device: nd.la has no such names, the reference's own are nd.concat / nd.stack. ---- */
  const lists = (name, plan) => function (axis, dtype, arrays) {
    if (arrays == null) {
      if (dtype == null) { arrays = axis; axis = undefined; }
      else { arrays = dtype; dtype = undefined; if (typeof axis === 'string') { dtype = axis; axis = undefined; } }
    }
    arrays = Array.from(arrays, asarray);
    if (!arrays.some(isDev)) throw new Error(`nd4hip.${name}: no device array among the arguments.`);
    const dt = dtypeOf(arrays[0]);
    if (!['float64', 'int32', 'complex128'].includes(dt) || arrays.some(a => dtypeOf(a) !== dt) || (dtype != null && dtype !== dt))
      throw new Error(`nd4hip.${name}: dtype is not accelerated.`);
    const pairs = dt === 'complex128', Cx = pairs ? (arrays.find(isDev)._complex || needComplex(name)) : null;
    const p = plan(axis, arrays.map(a => Array.from(a.shape))), shapes = p.shapes || arrays.map(a => Array.from(a.shape)), temps = [];
    const B = new DevBuf(p.shape.reduce((a, b) => a * b, 1) * (pairs ? 2 : 1), pairs || dt === 'float64' ? Float64Array : Int32Array);
    try {
      arrays.forEach((a, k) => {
        let buf = isDev(a) ? a._buf : null;
        if (!buf) { buf = DevBuf.from(pairs ? a.data._array : a.data); temps.push(buf); }
        gatherBox(B, p.offs[k], p.strides, buf, 0, cStrides(shapes[k]), shapes[k], pairs);
      });
    } catch (e) { B.free(); throw e; } finally { release(temps); }
    return new DeviceNDArray(Int32Array.from(p.shape), B, Cx);
  };
  for (const [name, plan] of [['concat', concatPlan], ['stack', stackPlan]]) {
    const f = lists(name, plan);
    Object.defineProperty(f, 'name', {value: name});
    Object.defineProperty(la, name, {value: f, writable: true, enumerable: false, configurable: true});
  }

  /* ---- zip_elems (zip_elems.js) on device arrays, csrc/elem.hip: (ndarrays, 'float64', zip_fn) as the reference's nd.zip_elems, for
   * the closures that are one IEEE operation on float64. zip_fn is an operator name ('add', 'sub', 'mul', 'div', 'min', 'max', 'neg',
   * 'abs') or a function identical to the host module's nd.math member (standalone: this package's `math`); the number of arrays
   * is the operator's arity (the reference appends the index to the arguments, so math.min over one array is no minimum). At least
   * one array must be a DeviceNDArray; host arrays and plain numbers (0-d) are uploaded on the way in. The result is a
   * DeviceNDArray. Not enumerable, like concat: nd.la has no such name, the reference's own is nd.zip_elems. ---- */
  const zip_elems = function (ndarrays, dtype, zip_fn) {
    if (zip_fn == null && typeof dtype === 'function') { zip_fn = dtype; dtype = undefined; }
    const arrays = Array.from(ndarrays, a => typeof a === 'number' ? {shape: new Int32Array(0), data: Float64Array.of(a)} : asarray(a));
    if (!arrays.some(isDev)) throw new Error('nd4hip.zip_elems: no device array among the arguments.');
    const op = ewName(zip_fn);
    if (op === null || EW_ARITY[op] !== arrays.length) throw new Error('nd4hip.zip_elems: zip_fn is not accelerated.');
    if (dtype !== 'float64' || arrays.some(a => dtypeOf(a) !== 'float64')) throw new Error('nd4hip.zip_elems: dtype is not accelerated.');
    const plan = zipPlan(arrays.map(a => a.shape)), temps = [];
    try {
      const bufs = arrays.map(a => { if (isDev(a)) return a._buf; const b = DevBuf.from(a.data); temps.push(b); return b; });
      return new DeviceNDArray(Int32Array.from(plan.shape), zipBox(op, plan, bufs));
    } finally { release(temps); }
  };
  Object.defineProperty(la, 'zip_elems', {value: zip_elems, writable: true, enumerable: false, configurable: true});

  /* ---- eigen_sym / eigenvals_sym, csrc/syev.hip: the functions the reference plans at eigen.js:28-30. S [..., N, N] float64, read
   * only in its lower triangle -> [eigenvalues [..., N] descending, eigenvectors [..., N, N] as columns], resp. the eigenvalues alone.
   * Host arrays or DeviceNDArrays in, the same kind out. Not enumerable, like concat: the reference's nd.la has no such names.
   * opts.algo: undefined / 'dc' (the default route) or 'jacobi' (csrc/syevj.hip, N <= 128: two-sided Jacobi in one launch, small
   * eigenvalues of a positive definite S to their own relative accuracy).
   * opts.subset: [i0, i1], 0 <= i0 < i1 <= N (not with 'jacobi'; an empty subset has no NDArray, whose axes are at least 1 long): the eigenvalues i0 .. i1 - 1 of the descending spectrum alone,
   * [..., k], and their eigenvectors, [..., N, k], k = i1 - i0, by bisection and inverse iteration (csrc/syevx.hip).
   * opts.reduction: undefined / 'hessenberg' (the default) or 'tridiag' (not with 'jacobi'): the symmetric tridiagonal reduction of
   * csrc/sytrd.hip under either route, the eigenvectors by its reflectors. ---- */
  /* ---- opts.interval = [lo, hi] (csrc/syevx.hip, DESIGN.md 4.22): the eigenvalues lo < lambda <= hi of every member. lo and hi are
   * numbers, or arrays / NDArrays with one entry per member in the order of the leading dimensions; lo <= hi, NaN is refused,
   * +-Infinity is a bound like any other. Results are ragged: [..., kmax] and [..., N, kmax], a member's own k_b pairs first, then
   * NaN / zero columns. The ranges (i0_b, i1_b) come back as the non-enumerable property `range` of the result (of the [L, V]
   * array, or of L where the values alone are asked for): int32 [..., 2], of the kind of the operands. An interval that holds no
   * eigenvalue of any member throws, as the empty subset does: an NDArray has no axis of length 0. ---- */
  const intervalBounds = (what, interval, batch) => {
    const bad = () => new Error(`${what}: interval must be [lo, hi] with lo <= hi, numbers or one entry per member.`);
    if (!(Array.isArray(interval) || ArrayBuffer.isView(interval)) || interval.length !== 2) throw bad();
    const side = x => {
      if (typeof x === 'number') return new Float64Array(batch).fill(x);
      const v = x != null && x.data != null ? x.data : x;
      if (!(Array.isArray(v) || ArrayBuffer.isView(v)) || (v.length !== batch && v.length !== 1) || Array.from(v).some(t => typeof t !== 'number')) throw bad();
      return v.length === batch ? Float64Array.from(v) : new Float64Array(batch).fill(v[0]);
    };
    const lo = side(interval[0]), hi = side(interval[1]), out = new Float64Array(2 * batch);
    for (let b = 0; b < batch; b++) {
      if (Number.isNaN(lo[b]) || Number.isNaN(hi[b])) throw new Error(`${what}: interval contains NaN.`);
      if (lo[b] > hi[b]) throw new Error(`${what}: interval must satisfy lo <= hi.`);
      out[2 * b] = lo[b]; out[2 * b + 1] = hi[b];
    }
    return out;
  };
  // the first k of kcap selected entries into a dense buffer [batch, R, k]; src element (b, r, j) at b sb + r sr + j sj
  const takeSelected = (dev, src, batch, R, k, sb, sr, sj) => {
    const out = alloc(dev, batch * R * k);
    if (dev) gatherBox(out, 0, [R * k, k, 1], src, 0, [sb, sr, sj], [batch, R, k], false);
    else for (let b = 0; b < batch; b++) for (let r = 0; r < R; r++) for (let j = 0; j < k; j++) out[(b * R + r) * k + j] = src[b * sb + r * sr + j * sj];
    return out;
  };
  const noneSelected = what => new Error(`${what}: the interval holds no eigenvalue of any member, and an NDArray has no axis of length 0.`);
  const withRange = (result, dev, lead, rg) => {
    const range = dev ? new DeviceNDArray(Int32Array.from(lead.concat([2])), rg) : new NDA(Int32Array.from(lead.concat([2])), rg);
    Object.defineProperty(result, 'range', {value: range, writable: true, enumerable: false, configurable: true});
    return result;
  };
  // one interval call with kcap = N and its ragged results cut to kmax: run(bounds, L, V, range) -> kmax; layout of the vectors:
  // 'cols' [batch, N, kcap] or 'rows' [batch, kcap, N]; both come back as [..., N, kmax]
  const intervalCall = (what, dev, lead, batch, N, interval, vectors, layout, run) => {
    const bounds = intervalBounds(what, interval, batch), temps = [];
    const L = alloc(dev, batch * N), V = vectors ? alloc(dev, batch * N * N) : null, rg = alloc(dev, batch * 2, Int32Array);
    const drop = () => { if (dev) { L.free(); if (V) V.free(); } };
    let k, Lk, Vk = null;
    try {
      let bd = bounds;
      if (dev) { bd = DevBuf.from(bounds); temps.push(bd); }
      k = run(view(bd, 0), view(L, 0), vectors ? view(V, 0) : null, view(rg, 0));
      if (k === 0) throw noneSelected(what);
      Lk = takeSelected(dev, L, batch, 1, k, N, 0, 1);
      if (vectors) Vk = layout === 'cols' ? takeSelected(dev, V, batch, N, k, N * N, N, 1) : takeSelected(dev, V, batch, N, k, N * N, 1, N);
    }
    catch (e) { if (dev) rg.free(); drop(); throw e; }
    finally { release(temps); }
    drop();
    const Lw = wrap(dev, lead.concat([k]), Lk);
    return withRange(vectors ? [Lw, wrap(dev, lead.concat([N, k]), Vk)] : Lw, dev, lead, rg);
  };

  const eigSym = (name, vectors) => {
    const f = function (S, opts) {
      const algo = opts == null ? undefined : opts.algo;
      if (algo !== undefined && algo !== null && algo !== 'dc' && algo !== 'jacobi') throw new Error(`${name}(S, {algo}): algo must be 'dc' or 'jacobi'.`);
      const jac = algo === 'jacobi';
      const reduction = opts == null ? undefined : opts.reduction;
      if (reduction !== undefined && reduction !== null && reduction !== 'hessenberg' && reduction !== 'tridiag')
        throw new Error(`${name}(S, {reduction}): reduction must be 'hessenberg' or 'tridiag'.`);
      const tr = reduction === 'tridiag';
      if (tr && jac) throw new Error(`${name}(S, {reduction}): reduction is not available with algo 'jacobi'.`);
      const subset = opts == null ? undefined : opts.subset;
      if (subset != null) {
        if (jac) throw new Error(`${name}(S, {subset}): subset is not available with algo 'jacobi'.`);
        if (!(Array.isArray(subset) || ArrayBuffer.isView(subset)) || subset.length !== 2)
          throw new Error(`${name}(S, {subset}): subset must be [i0, i1] with 0 <= i0 <= i1 <= N.`);
      }
      const interval = opts == null ? undefined : opts.interval;
      if (interval != null) {
        if (jac) throw new Error(`${name}(S, {interval}): interval is not available with algo 'jacobi'.`);
        if (subset != null) throw new Error(`${name}(S, {interval}): interval and subset exclude each other.`);
      }
      S = asarray(S);
      if (isComplexDev(S) || String(dtypeOf(S)).startsWith('complex')) throw new TypeError(`${name}(S): S.dtype must be float.`);
      if (S.ndim < 2) throw new Error(`${name}(S): S.ndim must be at least 2.`);
      const nd_ = S.ndim, N = S.shape[nd_ - 1];
      if (S.shape[nd_ - 2] != N) throw new Error(`${name}(S): S must be quadratic.`);
      if (!gpuOk(S)) throw new TypeError(`${name}(S): dtype ${dtypeOf(S)} is not accelerated.`);
      const batch = prod(S.shape, 0, nd_ - 2), dev = isDev(S), temps = [];
      if (interval != null) {                      // the same, the subset of each member chosen by value
        try {
          const Sd = opF64(S, dev, temps);
          return intervalCall(`${name}(S, {interval})`, dev, Array.from(S.shape.subarray(0, nd_ - 2)), batch, N, interval, vectors, 'cols',
                              (bd, L, V, rg) => native().dsyevxv_batched(tr ? 1 : 0, batch, N, N, bd, view(Sd, 0), L, V, rg));
        } finally { release(temps); }
      }
      if (subset != null) {                        // bisection and inverse iteration, csrc/syevx.hip
        const [i0, i1] = subset, k = i1 - i0;
        if (!(Number.isInteger(i0) && Number.isInteger(i1) && 0 <= i0 && i0 <= i1 && i1 <= N))
          throw new Error(`${name}(S, {subset}): subset must be [i0, i1] with 0 <= i0 <= i1 <= N, got [${i0}, ${i1}] for N = ${N}.`);
        if (k === 0) throw new Error(`${name}(S, {subset}): the subset [${i0}, ${i1}] is empty, and an NDArray has no axis of length 0.`);
        const lead = Array.from(S.shape.subarray(0, nd_ - 2));
        const Ls = alloc(dev, batch * k), Vs = vectors ? alloc(dev, batch * N * k) : null;
        try {
          if (vectors) native()[tr ? 'dsyevx_tr_batched' : 'dsyevx_batched'](batch, N, i0, i1, view(opF64(S, dev, temps), 0), view(Ls, 0), view(Vs, 0));
          else native()[tr ? 'dsyevxals_tr_batched' : 'dsyevxals_batched'](batch, N, i0, i1, view(opF64(S, dev, temps), 0), view(Ls, 0));
        }
        catch (e) { if (dev) { Ls.free(); if (Vs) Vs.free(); } throw e; }
        finally { release(temps); }
        const Lsw = wrap(dev, lead.concat([k]), Ls);
        return vectors ? [Lsw, wrap(dev, lead.concat([N, k]), Vs)] : Lsw;
      }
      const L = alloc(dev, batch * N), V = vectors ? alloc(dev, batch * N * N) : null;
      try {
        if (vectors) native()[tr ? 'dsyevd_tr_batched' : jac ? 'dsyevj_batched' : 'dsyevd_batched'](batch, N, view(opF64(S, dev, temps), 0), view(L, 0), view(V, 0));
        else native()[tr ? 'dsyevdals_tr_batched' : jac ? 'dsyevjals_batched' : 'dsyevals_batched'](batch, N, view(opF64(S, dev, temps), 0), view(L, 0));
      }
      catch (e) { if (dev) { L.free(); if (V) V.free(); } throw e; }
      finally { release(temps); }
      const Lw = wrap(dev, S.shape.subarray(0, nd_ - 1), L);
      return vectors ? [Lw, wrap(dev, S.shape, V)] : Lw;
    };
    Object.defineProperty(f, 'name', {value: name});
    Object.defineProperty(la, name, {value: f, writable: true, enumerable: false, configurable: true});
  };
  eigSym('eigen_sym', true); eigSym('eigenvals_sym', false);

  /* ---- eigen_herm / eigenvals_herm, csrc/hetrd.hip (DESIGN.md 4.24): H [..., N, N] complex128 Hermitian, read only where i >= j, the
   * imaginary part of its diagonal ignored, not written -> [eigenvalues float64 [..., N] descending, eigenvectors complex128
   * [..., N, N] as columns], resp. the eigenvalues alone (the same bits). Host arrays of the host module (install(nd): complex128
   * lives in its Complex128Array) or complex DeviceNDArrays in, the same kind out. opts.subset: [i0, i1] as for eigen_sym. A real
   * matrix is sent to eigen_sym. Not enumerable, like eigen_sym. ---- */
  const eigHerm = (name, vectors) => {
    const f = function (H, opts) {
      const subset = opts == null ? undefined : opts.subset;
      if (subset != null && (!(Array.isArray(subset) || ArrayBuffer.isView(subset)) || subset.length !== 2))
        throw new Error(`${name}(H, {subset}): subset must be [i0, i1] with 0 <= i0 <= i1 <= N.`);
      H = asarray(H);
      if (dtypeOf(H) !== 'complex128') throw new TypeError(`${name}(H): H.dtype must be complex128; a real symmetric matrix goes to eigen_sym.`);
      if (H.ndim < 2) throw new Error(`${name}(H): H.ndim must be at least 2.`);
      const nd_ = H.ndim, N = H.shape[nd_ - 1];
      if (H.shape[nd_ - 2] != N) throw new Error(`${name}(H): H must be quadratic.`);
      let i0 = 0, i1 = N;
      if (subset != null) {
        [i0, i1] = subset;
        if (!(Number.isInteger(i0) && Number.isInteger(i1) && 0 <= i0 && i0 <= i1 && i1 <= N))
          throw new Error(`${name}(H, {subset}): subset must be [i0, i1] with 0 <= i0 <= i1 <= N, got [${i0}, ${i1}] for N = ${N}.`);
        if (i1 === i0) throw new Error(`${name}(H, {subset}): the subset [${i0}, ${i1}] is empty, and an NDArray has no axis of length 0.`);
      }
      const Cx = needComplex(name);
      const k = i1 - i0, batch = prod(H.shape, 0, nd_ - 2), dev = isDev(H), temps = [], lead = Array.from(H.shape.subarray(0, nd_ - 2));
      const L = alloc(dev, batch * k), V = vectors ? alloc(dev, 2 * batch * N * k) : null;
      try {
        const Hd = view(opZ(H, dev, temps), 0);
        if (subset != null) {
          if (vectors) native().zheevx_batched(batch, N, i0, i1, Hd, view(L, 0), view(V, 0));
          else native().zheevxals_batched(batch, N, i0, i1, Hd, view(L, 0));
        }
        else if (vectors) native().zheevd_batched(batch, N, Hd, view(L, 0), view(V, 0));
        else native().zheevdals_batched(batch, N, Hd, view(L, 0));
      }
      catch (e) { if (dev) { L.free(); if (V) V.free(); } throw e; }
      finally { release(temps); }
      const Lw = wrap(dev, lead.concat([k]), L);
      if (!vectors) return Lw;
      const vs = Int32Array.from(lead.concat([N, k]));
      return [Lw, dev ? new DeviceNDArray(vs, V, Cx) : new NDA(vs, complexOver(Cx, V))];
    };
    Object.defineProperty(f, 'name', {value: name});
    Object.defineProperty(la, name, {value: f, writable: true, enumerable: false, configurable: true});
  };
  eigHerm('eigen_herm', true); eigHerm('eigenvals_herm', false);

  /* ---- herm_cholesky_decomp / herm_cholesky_solve / eigen_herm_gen / eigenvals_herm_gen, csrc/hegv.hip (DESIGN.md 4.25): complex128
   * operands of the host module (install(nd)) or complex DeviceNDArrays in, the same kind out. Hermitian operands are read only where
   * i >= j, the imaginary part of their diagonals is ignored, nothing is written. A real matrix is sent to the real function. Not
   * enumerable, like eigen_herm. ---- */
  const zSquare = (what, nm, M, goesTo) => {
    if (dtypeOf(M) !== 'complex128') throw new TypeError(`${what}: ${nm}.dtype must be complex128; a real symmetric matrix goes to ${goesTo}.`);
    if (M.ndim < 2) throw new Error(`${what}: ${nm}.ndim must be at least 2.`);
    if (M.shape[M.ndim - 2] != M.shape[M.ndim - 1]) throw new Error(`${what}: ${nm} must be quadratic.`);
    return M.shape[M.ndim - 1];
  };
  const zOut = (Cx, dev, shape, x) => dev ? new DeviceNDArray(Int32Array.from(shape), x, Cx) : new NDA(Int32Array.from(shape), complexOver(Cx, x));
  const hidden = (name, f) => {
    Object.defineProperty(f, 'name', {value: name});
    Object.defineProperty(la, name, {value: f, writable: true, enumerable: false, configurable: true});
  };
  // L [..., N, N] with H = L L^H: zeros above the diagonal, a real positive diagonal
  hidden('herm_cholesky_decomp', function (H) {
    const what = 'herm_cholesky_decomp(H)';
    H = asarray(H);
    const N = zSquare(what, 'H', H, 'cholesky_decomp'), Cx = needComplex('herm_cholesky_decomp');
    const batch = prod(H.shape, 0, H.ndim - 2), dev = isDev(H), temps = [], L = alloc(dev, 2 * batch * N * N);
    try { native().zpotrf_batched(batch, N, view(opZ(H, dev, temps), 0), view(L, 0)); }
    catch (e) { if (dev) L.free(); throw e; }
    finally { release(temps); }
    return zOut(Cx, dev, H.shape, L);
  });
  // X with L L^H X = Y; Y [..., N, K] complex128 or float64 (promoted); L has Y's leading dimensions or is exactly [N, N]
  hidden('herm_cholesky_solve', function (L, Y) {
    const what = 'herm_cholesky_solve(L,Y)';
    L = asarray(L); Y = asarray(Y);
    const N = zSquare(what, 'L', L, 'cholesky_solve'), Cx = needComplex('herm_cholesky_solve');
    const dy = dtypeOf(Y);
    if (dy !== 'complex128' && dy !== 'float64') throw new TypeError(`${what}: Y must be complex128 or float64.`);
    if (Y.ndim < 2) throw new Error(`${what}: Y.ndim must be at least 2.`);
    if (Y.shape[Y.ndim - 2] != N) throw new Error(`${what}: L and Y don't match.`);
    const K = Y.shape[Y.ndim - 1], leadY = Array.from(Y.shape.subarray(0, Y.ndim - 2)), leadL = Array.from(L.shape.subarray(0, L.ndim - 2));
    const same = leadL.length === leadY.length && leadL.every((s, i) => s == leadY[i]);
    if (!same && L.ndim !== 2) throw new Error(`${what}: L must have the leading dimensions of Y or be [N, N], got [${Array.from(L.shape)}] and [${Array.from(Y.shape)}].`);
    if (isDev(L) !== isDev(Y)) throw new TypeError(`${what}: L and Y must be both host arrays or both DeviceNDArrays.`);
    const batch = prod(Y.shape, 0, Y.ndim - 2), dev = isDev(L), temps = [], X = alloc(dev, 2 * batch * N * K);
    try {
      let y;
      if (dy === 'complex128') y = opZ(Y, dev, temps);
      else {                                     // a real Y: interleaved with zero imaginary parts on the host, then on the call's side
        const r = isDev(Y) ? la.to_host(Y).data : f64(Y), z = new Float64Array(2 * r.length);
        for (let i = 0; i < r.length; i++) z[2 * i] = r[i];
        if (dev) { y = DevBuf.from(z); temps.push(y); } else y = z;
      }
      native().zpotrs_batched(batch, N, K, view(opZ(L, dev, temps), 0), same ? N * N : 0, view(y, 0), view(X, 0));
    }
    catch (e) { if (dev) X.free(); throw e; }
    finally { release(temps); }
    return zOut(Cx, dev, Y.shape, X);
  });
  const eigHermGen = (name, vectors) => hidden(name, function (A, B, opts) {
    const what = `${name}(A,B)`;
    const subset = opts == null ? undefined : opts.subset;
    if (subset != null && (!(Array.isArray(subset) || ArrayBuffer.isView(subset)) || subset.length !== 2))
      throw new Error(`${name}(A,B, {subset}): subset must be [i0, i1] with 0 <= i0 <= i1 <= N.`);
    A = asarray(A); B = asarray(B);
    const N = zSquare(what, 'A', A, 'eigen_sym_gen');
    zSquare(what, 'B', B, 'eigen_sym_gen');
    const nd_ = A.ndim;
    const same = B.ndim === nd_ && A.shape.every((s, i) => s == B.shape[i]), one = !same && B.ndim === 2 && B.shape[0] == N && B.shape[1] == N;
    if (!same && !one) throw new Error(`${what}: B.shape must be A.shape or A.shape.slice(-2), got [${Array.from(B.shape)}] and [${Array.from(A.shape)}].`);
    if (isDev(A) !== isDev(B)) throw new TypeError(`${what}: A and B must be both host arrays or both DeviceNDArrays.`);
    let i0 = 0, i1 = N;
    if (subset != null) {
      [i0, i1] = subset;
      if (!(Number.isInteger(i0) && Number.isInteger(i1) && 0 <= i0 && i0 <= i1 && i1 <= N))
        throw new Error(`${name}(A,B, {subset}): subset must be [i0, i1] with 0 <= i0 <= i1 <= N, got [${i0}, ${i1}] for N = ${N}.`);
      if (i1 === i0) throw new Error(`${name}(A,B, {subset}): the subset [${i0}, ${i1}] is empty, and an NDArray has no axis of length 0.`);
    }
    const Cx = needComplex(name);
    const k = i1 - i0, batch = prod(A.shape, 0, nd_ - 2), dev = isDev(A), temps = [], lead = Array.from(A.shape.subarray(0, nd_ - 2)), sB = same ? N * N : 0;
    const L = alloc(dev, batch * k), X = vectors ? alloc(dev, 2 * batch * N * k) : null;
    try {
      const a = view(opZ(A, dev, temps), 0), b = view(opZ(B, dev, temps), 0);
      if (subset != null) {
        if (vectors) native().zhegvx_batched(batch, N, i0, i1, a, b, sB, view(L, 0), view(X, 0));
        else native().zhegvxals_batched(batch, N, i0, i1, a, b, sB, view(L, 0));
      }
      else if (vectors) native().zhegvd_batched(batch, N, a, b, sB, view(L, 0), view(X, 0));
      else native().zhegvals_batched(batch, N, a, b, sB, view(L, 0));
    }
    catch (e) { if (dev) { L.free(); if (X) X.free(); } throw e; }
    finally { release(temps); }
    const Lw = wrap(dev, lead.concat([k]), L);
    return vectors ? [Lw, zOut(Cx, dev, lead.concat([N, k]), X)] : Lw;
  });
  eigHermGen('eigen_herm_gen', true); eigHermGen('eigenvals_herm_gen', false);

  /* ---- eigen_sym_gen / eigenvals_sym_gen, csrc/sygv.hip: A x = lambda B x, A symmetric, B symmetric positive definite, both read
   * only in their lower triangles. A [..., N, N]; B of the same shape or exactly [N, N] (one B for every member, factorised once)
   * -> [eigenvalues [..., N] descending, eigenvectors [..., N, N] as columns with X^T B X = I], resp. the eigenvalues alone (the
   * same bits). Host arrays or DeviceNDArrays in (both of one kind), the same kind out. opts.algo as for eigen_sym. ---- */
  const eigSymGen = (name, vectors) => {
    const f = function (A, B, opts) {
      const algo = opts == null ? undefined : opts.algo;
      if (algo !== undefined && algo !== null && algo !== 'dc' && algo !== 'jacobi') throw new Error(`${name}(A,B, {algo}): algo must be 'dc' or 'jacobi'.`);
      // opts.subset, opts.interval and opts.reduction as for eigen_sym, applied to C = L^-1 A L^-T (not with 'jacobi'); the
      // back-transformation runs on the selected columns; an interval's ranges are the property `range` of the result
      const reduction = opts == null ? undefined : opts.reduction, subset = opts == null ? undefined : opts.subset, interval = opts == null ? undefined : opts.interval;
      if (reduction !== undefined && reduction !== null && reduction !== 'hessenberg' && reduction !== 'tridiag')
        throw new Error(`${name}(A,B, {reduction}): reduction must be 'hessenberg' or 'tridiag'.`);
      const tr = reduction === 'tridiag';
      for (const [kw, on] of [['reduction', tr], ['subset', subset != null], ['interval', interval != null]])
        if (on && algo === 'jacobi') throw new Error(`${name}(A,B, {${kw}}): ${kw} is not available with algo 'jacobi'.`);
      if (interval != null && subset != null) throw new Error(`${name}(A,B, {interval}): interval and subset exclude each other.`);
      if (subset != null && (!(Array.isArray(subset) || ArrayBuffer.isView(subset)) || subset.length !== 2))
        throw new Error(`${name}(A,B, {subset}): subset must be [i0, i1] with 0 <= i0 <= i1 <= N.`);
      A = asarray(A); B = asarray(B);
      for (const [nm, M] of [['A', A], ['B', B]]) {
        if (isComplexDev(M) || String(dtypeOf(M)).startsWith('complex')) throw new TypeError(`${name}(A,B): ${nm}.dtype must be float.`);
        if (M.ndim < 2) throw new Error(`${name}(A,B): ${nm}.ndim must be at least 2.`);
        if (M.shape[M.ndim - 2] != M.shape[M.ndim - 1]) throw new Error(`${name}(A,B): ${nm} must be quadratic.`);
        if (!gpuOk(M)) throw new TypeError(`${name}(A,B): dtype ${dtypeOf(M)} is not accelerated.`);
      }
      const nd_ = A.ndim, N = A.shape[nd_ - 1];
      const same = B.ndim === nd_ && A.shape.every((s, i) => s == B.shape[i]), one = !same && B.ndim === 2 && B.shape[0] == N && B.shape[1] == N;
      if (!same && !one) throw new Error(`${name}(A,B): B.shape must be A.shape or A.shape.slice(-2), got [${Array.from(B.shape)}] and [${Array.from(A.shape)}].`);
      if (isDev(A) !== isDev(B)) throw new TypeError(`${name}(A,B): A and B must be both host arrays or both DeviceNDArrays.`);
      const batch = prod(A.shape, 0, nd_ - 2), dev = isDev(A), temps = [], jac = algo === 'jacobi' ? 1 : 0;
      const lead = Array.from(A.shape.subarray(0, nd_ - 2)), sB = same ? N * N : 0;
      if (interval != null) {
        try {
          const a = view(opF64(A, dev, temps), 0), b = view(opF64(B, dev, temps), 0);
          return intervalCall(`${name}(A,B, {interval})`, dev, lead, batch, N, interval, vectors, 'cols',
                              (bd, L, X, rg) => native().dsygvx_batched(tr ? 1 : 0, 2, batch, N, 0, 0, N, bd, a, b, sB, L, X, rg));
        } finally { release(temps); }
      }
      if (subset != null || tr) {
        let i0 = 0, i1 = N;
        if (subset != null) {
          [i0, i1] = subset;
          if (!(Number.isInteger(i0) && Number.isInteger(i1) && 0 <= i0 && i0 <= i1 && i1 <= N))
            throw new Error(`${name}(A,B, {subset}): subset must be [i0, i1] with 0 <= i0 <= i1 <= N, got [${i0}, ${i1}] for N = ${N}.`);
          if (i1 === i0) throw new Error(`${name}(A,B, {subset}): the subset [${i0}, ${i1}] is empty, and an NDArray has no axis of length 0.`);
        }
        const k = i1 - i0, Ls = alloc(dev, batch * k), Xs = vectors ? alloc(dev, batch * N * k) : null;
        try {
          native().dsygvx_batched(tr ? 1 : 0, subset != null ? 1 : 0, batch, N, i0, i1, 0, null, view(opF64(A, dev, temps), 0), view(opF64(B, dev, temps), 0), sB,
                                  view(Ls, 0), vectors ? view(Xs, 0) : null, null);
        }
        catch (e) { if (dev) { Ls.free(); if (Xs) Xs.free(); } throw e; }
        finally { release(temps); }
        const Lsw = wrap(dev, lead.concat([k]), Ls);
        return vectors ? [Lsw, wrap(dev, lead.concat([N, k]), Xs)] : Lsw;
      }
      const L = alloc(dev, batch * N), X = vectors ? alloc(dev, batch * N * N) : null;
      try {
        const a = view(opF64(A, dev, temps), 0), b = view(opF64(B, dev, temps), 0);
        if (vectors) native().dsygvd_batched(jac, batch, N, a, b, same ? N * N : 0, view(L, 0), view(X, 0));
        else native().dsygvals_batched(jac, batch, N, a, b, same ? N * N : 0, view(L, 0));
      }
      catch (e) { if (dev) { L.free(); if (X) X.free(); } throw e; }
      finally { release(temps); }
      const Lw = wrap(dev, A.shape.subarray(0, nd_ - 1), L);
      return vectors ? [Lw, wrap(dev, A.shape, X)] : Lw;
    };
    Object.defineProperty(f, 'name', {value: name});
    Object.defineProperty(la, name, {value: f, writable: true, enumerable: false, configurable: true});
  };
  eigSymGen('eigen_sym_gen', true); eigSymGen('eigenvals_sym_gen', false);

  /* ---- tridiag_eigen(d, e, opts) / tridiag_eigenvals(d, e, opts) / tridiag_count(d, e, x), csrc/syevx.hip: the symmetric tridiagonal T
   * with diagonal d [..., N] and off-diagonal e [..., N-1] (N = 1: e is null, an NDArray has no axis of length 0), N <= 2048.
   * opts.subset = [i0, i1] (default: all) or opts.interval = [lo, hi] as for eigen_sym -> [L [..., k] descending, Z [..., N, k] with the
   * eigenvectors as columns], resp. L alone; tridiag_count -> int32 [..., M], how many eigenvalues are greater than each x [..., M].
   * Host arrays or DeviceNDArrays in (all of one kind), the same kind out. Not enumerable, like eigen_sym. ---- */
  const tridiagArgs = (what, d, e, extra) => {
    d = asarray(d); e = e == null ? null : asarray(e);
    const all = [d].concat(e ? [e] : []).concat(extra ? [extra] : []);
    for (const M of all) {
      if (isComplexDev(M) || String(dtypeOf(M)).startsWith('complex')) throw new TypeError(`${what}: the operands must be float.`);
      if (!gpuOk(M)) throw new TypeError(`${what}: dtype ${dtypeOf(M)} is not accelerated.`);
    }
    if (all.some(M => isDev(M) !== isDev(d))) throw new TypeError(`${what}: the operands must be all host arrays or all DeviceNDArrays.`);
    const nd_ = d.ndim, N = d.shape[nd_ - 1], lead = Array.from(d.shape.subarray(0, nd_ - 1));
    if (N > 2048) throw new Error(`${what}: N <= 2048.`);
    if (N === 1 ? e != null : (e == null || e.ndim !== nd_ || e.shape[nd_ - 1] !== N - 1 || lead.some((s, i) => s != e.shape[i])))
      throw new Error(`${what}: e must have the leading dimensions of d and len(d) - 1 entries (null for N = 1).`);
    return {d, e, N, lead, batch: lead.reduce((p, q) => p * q, 1), dev: isDev(d)};
  };
  const tridiagEigen = (name, vectors) => {
    const f = function (d, e, opts) {
      const what = `${name}(d,e)`, subset = opts == null ? undefined : opts.subset, interval = opts == null ? undefined : opts.interval;
      if (interval != null && subset != null) throw new Error(`${what}: interval and subset exclude each other.`);
      if (subset != null && (!(Array.isArray(subset) || ArrayBuffer.isView(subset)) || subset.length !== 2))
        throw new Error(`${what}: subset must be [i0, i1] with 0 <= i0 <= i1 <= N.`);
      const t = tridiagArgs(what, d, e), {N, lead, batch, dev} = t, temps = [];
      try {
        const dd = view(opF64(t.d, dev, temps), 0), ee = t.e ? view(opF64(t.e, dev, temps), 0) : null;
        if (interval != null)
          return intervalCall(`${what}`, dev, lead, batch, N, interval, vectors, 'rows', (bd, L, Z, rg) => native().dstevxv_batched(batch, N, N, bd, dd, ee, L, Z, rg));
        const [i0, i1] = subset != null ? subset : [0, N], k = i1 - i0;
        if (!(Number.isInteger(i0) && Number.isInteger(i1) && 0 <= i0 && i0 <= i1 && i1 <= N))
          throw new Error(`${what}: subset must be [i0, i1] with 0 <= i0 <= i1 <= N, got [${i0}, ${i1}] for N = ${N}.`);
        if (k === 0) throw new Error(`${what}: the subset [${i0}, ${i1}] is empty, and an NDArray has no axis of length 0.`);
        const L = alloc(dev, batch * k), Z = vectors ? alloc(dev, batch * k * N) : null;
        let Zt = null;
        try {
          native().dstevx_batched(batch, N, i0, i1, dd, ee, view(L, 0), vectors ? view(Z, 0) : null);
          if (vectors) Zt = takeSelected(dev, Z, batch, N, k, k * N, 1, N);      // rows = vectors -> columns
        }
        catch (err) { if (dev) L.free(); throw err; }
        finally { if (dev && Z) Z.free(); }
        const Lw = wrap(dev, lead.concat([k]), L);
        return vectors ? [Lw, wrap(dev, lead.concat([N, k]), Zt)] : Lw;
      } finally { release(temps); }
    };
    Object.defineProperty(f, 'name', {value: name});
    Object.defineProperty(la, name, {value: f, writable: true, enumerable: false, configurable: true});
  };
  tridiagEigen('tridiag_eigen', true); tridiagEigen('tridiag_eigenvals', false);
  const tridiag_count = function (d, e, x) {
    const what = 'tridiag_count(d,e,x)';
    x = asarray(x);
    const t = tridiagArgs(what, d, e, x), {N, lead, batch, dev} = t, temps = [];
    if (x.ndim !== lead.length + 1 || lead.some((s, i) => s != x.shape[i])) throw new Error(`${what}: x must have the leading dimensions of d.`);
    const M = x.shape[x.ndim - 1];
    if (!dev && Array.from(f64(x)).some(Number.isNaN)) throw new Error(`${what}: x contains NaN.`);
    const count = alloc(dev, batch * M, Int32Array);
    try {
      native().dstcnt_batched(batch, N, M, view(opF64(t.d, dev, temps), 0), t.e ? view(opF64(t.e, dev, temps), 0) : null, view(opF64(x, dev, temps), 0), view(count, 0));
    }
    catch (err) { if (dev) count.free(); throw err; }
    finally { release(temps); }
    return wrap(dev, lead.concat([M]), count);
  };
  Object.defineProperty(la, 'tridiag_count', {value: tridiag_count, writable: true, enumerable: false, configurable: true});

  // complex128 device arrays are accepted by matmul2 / matmul only: every other function refuses them before it looks at the
  // buffer (which holds 2n doubles, not n float64 entries)
  const complexOk = new Set(['matmul2', 'matmul', 'eigen_balance_post', '_chain_plan', 'to_device', 'to_host', 'synchronize', 'profile_enable', 'profile_last']);
  for (const k of Object.keys(la)) {
    const f = la[k];
    if (typeof f !== 'function' || complexOk.has(k) || f === DeviceNDArray || f === SolveError) continue;   // (classes stay as they are)
    const g = function (...args) {
      if (args.some(x => isComplexDev(x) || (Array.isArray(x) && x.some(isComplexDev))))
        throw new Error(`nd4hip.${k}: complex128 device arrays are not accelerated (only matmul2 and matmul take them).`);
      return f.apply(this, args);
    };
    Object.defineProperty(g, 'name', {value: f.name});
    la[k] = g;
  }
  return la;
}

const standalone = makeLa(NDArray, null, SingularMatrixSolveError, null);

// estimated work of a call (flops, SURVEY.md 8d conventions up to a constant): what install(nd, {minWork}) compares with
function estimatedWork(name, args) {
  const dims = a => { const s = a && a.shape ? Array.from(a.shape) : null; if (!s || s.length < 2) return null;
                      let b = 1; for (let i = 0; i < s.length - 2; i++) b *= s[i]; return [b, s[s.length - 2], s[s.length - 1]]; };
  if (name === 'urv_lstsq' && Array.isArray(args[0])) args = args[0];   // urv_lstsq([U,R,V,ranks], Y): the work of U
  if (name === 'norm') { const x = args[0]; return x && x.shape ? Array.from(x.shape).reduce((p, q) => p * q, 1) : Infinity; }   // its size
  const a = dims(args[0]);
  if (a && (name === 'det_tri' || name === 'slogdet_tri')) return a[0] * a[1];                   // N per matrix
  if (!a) return Infinity;                                  // nested JS arrays etc.: let the accelerated path coerce them
  // real flops of one product: 2 IKJ real, 8 IKJ complex x complex, 4 IKJ mixed
  const cx = x => !!x && x.dtype === 'complex128', fl = (x, y) => cx(x) && cx(y) ? 8 : cx(x) || cx(y) ? 4 : 2;
  if (name === 'matmul2') { const b = dims(args[1]); return b ? fl(args[0], args[1]) * Math.max(a[0], b[0]) * a[1] * a[2] * b[2] : Infinity; }
  if (name === 'matmul') { let w = 0; for (let i = 0; i + 1 < args.length; i++) { const x = dims(args[i]), y = dims(args[i + 1]); if (!x || !y) return Infinity; w += fl(args[i], args[i + 1]) * Math.max(x[0], y[0]) * x[1] * x[2] * y[2]; } return w; }
  return a[0] * a[1] * a[2] * Math.min(a[1], a[2]);
}

// schur_decomp, eigen, eigenvals of ONE host matrix: the host module's single thread wins up to N = 128 (64: 6.2 ms against
// 10.2 ms through the device with copies, 128: 40.5 against 50.8), the device from 256 on (429 against 226 ms); DESIGN.md §4.12
const SCHUR_ROUTED = new Set(['schur_decomp', 'eigen', 'eigenvals']), SCHUR_HOST_MAX_N = 128;
// the structure functions run on the device only for device-resident arguments (a host array would pay two PCIe crossings to be copied)
const STRUCT_ROUTED = new Set(['tril', 'triu', 'diag', 'diag_mat', 'permute_rows', 'permute_cols', 'unpermute_rows', 'unpermute_cols']);

/** Patch a loaded nd4js instance in place: the hot-path functions run on the GPU. Returns nd.
 *  opts.minWork (default 0 = off): a call whose estimated work (flops: 2 I K J for products, M N min(M, N) per matrix for
 *  decompositions and solves) is below it — and whose operands all live on the host — is forwarded to the HOST MODULE'S OWN
 *  function (`nd.la.*` as it was before install; never to this repo's oracle): one tiny matrix costs 50 us - 1 ms through any GPU
 *  path (the reference's own suites live at N <= 161: _generic_test_svd_decomp.js:308-336, lu_test.js:82-94). */
function install(nd, opts) {
  if (!nd || !nd.la || !nd.NDArray) throw new Error('nd4hip.install(nd): pass the nd4js module.');
  const minWork = opts && opts.minWork > 0 ? +opts.minWork : 0;
  const original = {matmul2: nd.la.matmul2, matmul: nd.la.matmul, qr_decomp: nd.la.qr_decomp, qr_decomp_full: nd.la.qr_decomp_full,
                    lu_decomp: nd.la.lu_decomp, svd_decomp: nd.la.svd_decomp, svd_dc: nd.la.svd_dc,
                    lu_solve: nd.la.lu_solve, tril_solve: nd.la.tril_solve, triu_solve: nd.la.triu_solve,
                    qr_lstsq: nd.la.qr_lstsq, svd_lstsq: nd.la.svd_lstsq, svd_solve: nd.la.svd_solve, svd_rank: nd.la.svd_rank,
                    cholesky_decomp: nd.la.cholesky_decomp, cholesky_solve: nd.la.cholesky_solve,
                    ldl_decomp: nd.la.ldl_decomp, ldl_solve: nd.la.ldl_solve,
                    pldlp_decomp: nd.la.pldlp_decomp, pldlp_solve: nd.la.pldlp_solve, pldlp_l: nd.la.pldlp_l, pldlp_d: nd.la.pldlp_d, pldlp_p: nd.la.pldlp_p,
                    hessenberg_decomp: nd.la.hessenberg_decomp, bidiag_decomp: nd.la.bidiag_decomp,
                    rrqr_decomp: nd.la.rrqr_decomp, rrqr_decomp_full: nd.la.rrqr_decomp_full, rrqr_rank: nd.la.rrqr_rank,
                    rrqr_lstsq: nd.la.rrqr_lstsq, rrqr_solve: nd.la.rrqr_solve, solve: nd.la.solve,
                    srrqr_decomp_full: nd.la.srrqr_decomp_full, urv_decomp_full: nd.la.urv_decomp_full, urv_lstsq: nd.la.urv_lstsq,
                    det: nd.la.det, slogdet: nd.la.slogdet, det_tri: nd.la.det_tri, slogdet_tri: nd.la.slogdet_tri,
                    rank: nd.la.rank, lstsq: nd.la.lstsq, norm: nd.la.norm,
                    schur_eigenvals: nd.la.schur_eigenvals, schur_eigen: nd.la.schur_eigen,
                    eigen_balance_pre: nd.la.eigen_balance_pre, eigen_balance_post: nd.la.eigen_balance_post,
                    schur_decomp: nd.la.schur_decomp, eigen: nd.la.eigen, eigenvals: nd.la.eigenvals,
                    tril: nd.la.tril, triu: nd.la.triu, diag: nd.la.diag, diag_mat: nd.la.diag_mat,
                    permute_rows: nd.la.permute_rows, permute_cols: nd.la.permute_cols,
                    unpermute_rows: nd.la.unpermute_rows, unpermute_cols: nd.la.unpermute_cols};
  if (nd.math && !mathTables.includes(nd.math)) mathTables.push(nd.math);       // its closures name the device operators (zip_elems, mapElems, reduceElems)
  const acc = makeLa(nd.NDArray, original, nd.la.SingularMatrixSolveError || SingularMatrixSolveError, (nd.dt && nd.dt.Complex128Array) || null);
  const target = Object.isFrozen(nd.la) || !Object.getOwnPropertyDescriptor(nd.la, 'matmul2').writable ? null : nd.la;
  const patched = target || Object.create(nd.la);
  const route = k => {
    if (SCHUR_ROUTED.has(k) && typeof original[k] === 'function') {
      const f = function (...args) {                      // one host matrix up to the crossover is the host module's (DESIGN.md §4.12)
        const A = args[0], s = A && A.shape, single = !!s && s.length >= 2 && Array.from(s).slice(0, -2).every(x => x === 1);
        const onHost = !(A instanceof acc.DeviceNDArray);
        if (onHost && single && s[s.length - 1] <= SCHUR_HOST_MAX_N) return original[k].apply(nd.la, args);
        return onHost && minWork && estimatedWork(k, args) < minWork ? original[k].apply(nd.la, args) : acc[k](...args);
      };
      Object.defineProperty(f, 'name', {value: k});
      return f;
    }
    if (STRUCT_ROUTED.has(k) && typeof original[k] === 'function') {
      // pure data movement: a call without a device argument is the host module's own, untouched (every dtype, whatever minWork
      // says); a device argument keeps the chain on the device
      const f = function (...args) {
        return args.some(x => x instanceof acc.DeviceNDArray) ? acc[k](...args) : original[k].apply(nd.la, args);
      };
      Object.defineProperty(f, 'name', {value: k});
      return f;
    }
    if (!minWork || typeof original[k] !== 'function') return acc[k];
    const f = function (...args) {
      const onHost = args.every(x => !(x instanceof acc.DeviceNDArray));
      return onHost && estimatedWork(k, args) < minWork ? original[k].apply(nd.la, args) : acc[k](...args);
    };
    Object.defineProperty(f, 'name', {value: k});
    return f;
  };
  for (const k of Object.keys(original)) Object.defineProperty(patched, k, {value: route(k), writable: true, enumerable: true, configurable: true});
  for (const k of ['to_device', 'to_host', 'synchronize', 'DeviceNDArray', 'profile_enable', 'profile_last', 'schur_qrfrancis', 'concat', 'stack', 'zip_elems', 'eigen_sym', 'eigenvals_sym', 'eigen_sym_gen', 'eigenvals_sym_gen', 'eigen_herm', 'eigenvals_herm', 'herm_cholesky_decomp', 'herm_cholesky_solve', 'eigen_herm_gen', 'eigenvals_herm_gen'])   // §8f N3 / §8b extensions, not in the reference (schur_qrfrancis: its private step)
    Object.defineProperty(patched, k, {value: acc[k], writable: true, enumerable: false, configurable: true});
  if (!target) { try { nd.la = patched; } catch (e) { /* exported getter: caller uses the returned object */ } }
  patched.__nd4hip_original__ = original;
  if (target) return nd;
  const out = Object.create(nd);
  Object.defineProperty(out, 'la', {value: patched, enumerable: true, writable: true, configurable: true});
  return out;
}

module.exports = Object.assign(standalone, {
  NDArray, DeviceNDArray, SingularMatrixSolveError, install, bcastGroups, complexOver,
  slicePlan, transposePlan, reshapeShape, concatPlan, stackPlan, reduceBox, zipPlan, reducePlan, math,
  accelerated: a => !!a && (isDev(a) || a.data instanceof Float64Array || a.data instanceof Int32Array),
  device_count: () => native().device_count(),
  devices: () => native().devices(),            // ids behind the handle (ND4HIP_DEVICES=all|0,1,...: batched host calls are sharded)
  version: () => native().version(),
});
