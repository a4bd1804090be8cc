'use strict';
/* Node-side checks of sliceElems, transpose(...axes) and reshape on DeviceNDArray and of la.concat / la.stack through the JS host
 * and the N-API addon. Driven by tests/test_node_slice.py. Everything moves words and never computes: comparisons are of the
 * 32-bit words of the buffers, exact.
 *   node node_slice_checks.js cpu <golden dir>                  (no GPU: the JS planners evaluated on the host against every fixture,
 *                                                                every refusal of the manifest with its recorded text, concat / stack
 *                                                                without a device array)
 *   node node_slice_checks.js install <reference dist/nd.js>    (la.concat / la.stack present and not enumerable after install,
 *                                                                nd.concat / nd.stack untouched)
 *   node node_slice_checks.js gpu <golden dir>                  (GPU: every fixture on device arrays of the three dtypes, a host array
 *                                                                mixed into a list, a truncated SVD that never leaves the device,
 *                                                                reshape and dispose; never reads the reference)
 */
const fs = require('fs'), path = require('path');
const la = require(path.join(__dirname, '..', '..', 'nd4js_amd', 'js'));
const assert = require('assert');
const mode = process.argv[2];

function loadNpy(file) {
  const buf = fs.readFileSync(file), hlen = buf.readUInt16LE(8), hdr = buf.toString('latin1', 10, 10 + hlen);
  const descr = /'descr': '([^']+)'/.exec(hdr)[1], shape = /'shape': \(([^)]*)\)/.exec(hdr)[1].split(',').filter(x => x.trim()).map(Number);
  const body = buf.slice(10 + hlen), ab = body.buffer.slice(body.byteOffset, body.byteOffset + body.byteLength);
  const dtype = {'<i4': 'int32', '<f8': 'float64', '<c16': 'complex128'}[descr];
  return {data: dtype === 'int32' ? new Int32Array(ab) : new Float64Array(ab), shape, dtype};      // complex128: interleaved (re, im)
}
const words = t => new Uint32Array(t.buffer, t.byteOffset, t.byteLength / 4);
function sameWords(a, b, what) {
  assert.strictEqual(a.constructor, b.constructor, what);
  const x = words(a), y = words(b);
  assert.strictEqual(x.length, y.length, what);
  for (let i = 0; i < x.length; i++) assert(x[i] === y[i], `${what}: 32-bit word ${i} is ${x[i]}, the reference has ${y[i]}`);
}
const prod = s => s.reduce((x, y) => x * y, 1);
function fixtures(dir) {
  const G = path.join(dir, 'slice'), m = JSON.parse(fs.readFileSync(path.join(G, 'manifest.json')));
  return {m, load: entry => loadNpy(path.join(G, entry.file))};
}
const inputsOf = (m, load, c) => (c.arrays || [c.A]).map(n => load(m.inputs[n]));
const rowMajor = shape => { const st = new Array(shape.length); let s = 1; for (let d = shape.length - 1; d >= 0; d--) { st[d] = s; s *= shape[d]; } return st; };

// dst[dstOff + sum i_d ds[d]] = src[srcOff + sum i_d ss[d]] in units of `w` words, on host typed arrays
function copyBox(dst, dstOff, ds, src, srcOff, ss, shape, w) {
  const n = prod(shape), idx = new Array(shape.length).fill(0);
  for (let e = 0; e < n; e++) {
    let so = srcOff, dof = dstOff;
    for (let d = 0; d < shape.length; d++) { so += idx[d] * ss[d]; dof += idx[d] * ds[d]; }
    assert(so >= 0 && so * w + w <= src.length && dof >= 0 && dof * w + w <= dst.length, 'the plan leaves its operand');
    for (let k = 0; k < w; k++) dst[dof * w + k] = src[so * w + k];
    for (let d = shape.length - 1; d >= 0; d--) { if (++idx[d] < shape[d]) break; idx[d] = 0; }
  }
}
// one recorded call from the JS planners alone, through reduceBox as the device path goes: {shape, data}
function planned(c, ins) {
  const w = ins[0].dtype === 'complex128' ? 2 : 1, Ctor = ins[0].data.constructor;
  const run = (dst, dstOff, ds, src, srcOff, ss, shape) => {
    const box = la.reduceBox(shape, ss, ds);
    assert(box.shape.length <= 8);
    for (const [so, dof] of box.loop) copyBox(dst, dstOff + dof, box.ds, src, srcOff + so, box.ss, box.shape, w);
  };
  if (c.fn === 'sliceElems') {
    const p = la.slicePlan(ins[0].shape, c.slices), out = new Ctor(prod(p.shape) * w);
    run(out, 0, rowMajor(p.shape), ins[0].data, p.off, p.strides, p.shape);
    return {shape: p.shape, data: out};
  }
  if (c.fn === 'transpose') {
    const p = la.transposePlan(ins[0].shape, c.axes), out = new Ctor(prod(p.shape) * w);
    run(out, 0, rowMajor(p.shape), ins[0].data, 0, p.strides, p.shape);
    return {shape: p.shape, data: out};
  }
  if (c.fn === 'reshape') return {shape: la.reshapeShape(ins[0].shape, prod(ins[0].shape), c.shape), data: ins[0].data};
  const shapes = ins.map(a => a.shape), p = c.fn === 'concat' ? la.concatPlan(c.axis, shapes) : la.stackPlan(c.axis, shapes);
  const out = new Ctor(prod(p.shape) * w);
  ins.forEach((a, k) => { const sh = (p.shapes || shapes)[k]; run(out, p.offs[k], p.strides, a.data, 0, rowMajor(sh), sh); });
  return {shape: p.shape, data: out};
}
function refusedCall(e) {
  if (e.fn === 'sliceElems') return () => la.slicePlan(e.a_shape, e.slices);
  if (e.fn === 'transpose') return () => la.transposePlan(e.a_shape, e.axes);
  if (e.fn === 'reshape') return () => la.reshapeShape(e.a_shape, prod(e.a_shape), e.shape);
  return () => (e.fn === 'concat' ? la.concatPlan : la.stackPlan)(e.axis, e.shapes);
}

if (mode === 'cpu') {
  const {m, load} = fixtures(process.argv[3]);
  let n = 0;
  for (const name of Object.keys(m.cases)) {
    const c = m.cases[name], want = load(c.out), got = planned(c, inputsOf(m, load, c));
    assert.deepStrictEqual(Array.from(got.shape), want.shape, name);
    sameWords(got.data, want.data, name);
    n++;
  }
  assert(n >= 150);
  for (const e of m.errors) assert.throws(refusedCall(e), err => err.message === e.message, `${e.fn} ${JSON.stringify(e)}: expected "${e.message}"`);
  assert(m.errors.length >= 30);
  // a 10-axis box of extent 2 with a step on every axis: 8 axes for the kernel and a loop of 4
  { const p = la.slicePlan(new Array(10).fill(4), new Array(10).fill([null, null, 2])), box = la.reduceBox(p.shape, p.strides, rowMajor(p.shape));
    assert.deepStrictEqual(box.shape, new Array(8).fill(2)); assert.strictEqual(box.loop.length, 4); }
  assert.deepStrictEqual(la.reduceBox([3, 4, 5], [20, 5, 1], [20, 5, 1]), {shape: [60], ss: [1], ds: [1], loop: [[0, 0]]});
  // the methods exist; without a device array the two list functions refuse, before anything touches a device
  for (const k of ['sliceElems', 'transpose', 'reshape']) assert.strictEqual(typeof la.DeviceNDArray.prototype[k], 'function', k);
  const h = new la.NDArray(Int32Array.of(2, 2), Float64Array.of(1, 2, 3, 4));
  for (const fn of ['concat', 'stack']) {
    assert.strictEqual(la[fn].name, fn);
    assert(!Object.keys(la).includes(fn), fn + ' must not be enumerable');
    for (const args of [[[h, h]], [0, [h, h]], [1, 'float64', [h]], ['float64', [h, h]]])
      assert.throws(() => la[fn](...args), err => err.message === `nd4hip.${fn}: no device array among the arguments.`, fn);
  }
  console.log('node slice cpu checks ok');
} else if (mode === 'install') {
  const nd = require(process.argv[3]);
  const before = {concat: nd.concat, stack: nd.stack, laKeys: Object.keys(nd.la).length};
  const out = la.install(nd), L = out.la;
  for (const fn of ['concat', 'stack']) {
    assert.strictEqual(typeof L[fn], 'function', fn);
    assert.strictEqual(L[fn].name, fn);
    assert(!Object.keys(L).includes(fn) && !Object.prototype.propertyIsEnumerable.call(L, fn), fn + ' must not be enumerable');
    assert.strictEqual(out[fn], before[fn], `nd.${fn} must stay the host module's`);
    assert.strictEqual(nd[fn], before[fn]);
    const A = nd.array('float64', [[1, 2], [3, 4]]);
    assert.throws(() => L[fn]([A, A]), err => err.message === `nd4hip.${fn}: no device array among the arguments.`);
  }
  assert(!Object.keys(L).includes('to_device'));
  // the host module's own concat and stack still answer host arrays
  const A = nd.array('int32', [[1, 2], [3, 4]]);
  assert.deepStrictEqual(Array.from(nd.concat(1, [A, A]).shape), [2, 4]);
  assert.deepStrictEqual(Array.from(nd.stack(-1, [A, A]).shape), [2, 2, 2]);
  console.log('node slice install checks ok');
} else if (mode === 'gpu') {
  // a host module's complex array, as far as this package looks at it: (buffer, byteOffset, length in complex elements), `_array`
  class CxArray { constructor(buffer, byteOffset, length) { this._array = new Float64Array(buffer, byteOffset, 2 * length); this.length = length; } }
  class HostNDArray {
    constructor(shape, data) { this.shape = shape; this.data = data; }
    get ndim() { return this.shape.length; }
    get dtype() { return this.data instanceof CxArray ? 'complex128' : this.data instanceof Float64Array ? 'float64' : this.data instanceof Int32Array ? 'int32' : 'object'; }
  }
  const L = la.install({NDArray: HostNDArray, la: {matmul2: () => 'host'}, dt: {Complex128Array: CxArray}}).la;
  const {m, load} = fixtures(process.argv[3]);
  const host = x => new HostNDArray(Int32Array.from(x.shape), x.dtype === 'complex128' ? new CxArray(x.data.buffer, x.data.byteOffset, x.data.length / 2) : x.data);
  const raw = d => d.dtype === 'complex128' ? d.data._array : d.data;
  const seen = {float64: 0, int32: 0, complex128: 0};
  for (const name of Object.keys(m.cases)) {
    const c = m.cases[name], want = load(c.out), ins = inputsOf(m, load, c), devs = ins.map(a => L.to_device(host(a)));
    let got;
    if (c.fn === 'sliceElems') got = devs[0].sliceElems(...c.slices);
    else if (c.fn === 'transpose') {
      if (c.axes.length === 0 && ins[0].dtype !== 'float64') { assert.throws(() => devs[0].transpose(), /^Error: nd4hip\.T: .* not accelerated\.$/, name); continue; }
      got = devs[0].transpose(...c.axes);
    } else if (c.fn === 'reshape') got = devs[0].reshape(...c.shape);
    else got = c.axis === null ? L[c.fn](devs) : L[c.fn](c.axis, devs);
    assert(got instanceof L.DeviceNDArray && devs.every(d => d._host === null) && got._host === null, name + ': a device call downloaded');
    assert.strictEqual(got.dtype, want.dtype, name);
    assert.deepStrictEqual(Array.from(got.shape), want.shape, name);
    sameWords(raw(got), want.data, name);
    seen[want.dtype]++;
  }
  assert(seen.float64 >= 50 && seen.int32 >= 40 && seen.complex128 >= 40, JSON.stringify(seen));
  // a host array mixed into a list is uploaded on the way in; dtype given and equal; mismatches are refused, never converted
  { const c = m.cases.concat_A_cols_ax1, ins = inputsOf(m, load, c), want = load(c.out);
    const mixed = [host(ins[0]), L.to_device(host(ins[1])), host(ins[2])];
    sameWords(L.concat(1, 'float64', mixed).data, want.data, 'concat with host arrays in the list');
    assert.throws(() => L.concat(1, 'int32', mixed), /^Error: nd4hip\.concat: dtype is not accelerated\.$/);
    const I = host({shape: ins[0].shape, dtype: 'int32', data: new Int32Array(prod(ins[0].shape))});
    assert.throws(() => L.concat(1, [L.to_device(host(ins[0])), I]), /^Error: nd4hip\.concat: dtype is not accelerated\.$/);
    assert.throws(() => L.stack([L.to_device(host(ins[0])), host(ins[1])]), err => err.message === 'Shape along all axes but the concatentation axis must match.'); }
  // refusals on device arrays carry the recorded texts
  { const dA = L.to_device(host({shape: [4, 6], dtype: 'float64', data: new Float64Array(24)}));
    for (const e of m.errors) {
      if (e.fn === 'sliceElems') assert.throws(() => dA.sliceElems(...e.slices), err => err.message === e.message, JSON.stringify(e));
      if (e.fn === 'transpose') assert.throws(() => dA.transpose(...e.axes), err => err.message === e.message, JSON.stringify(e));
      if (e.fn === 'reshape') assert.throws(() => dA.reshape(...e.shape), err => err.message === e.message, JSON.stringify(e));
    } }
  // a truncated SVD that never reads .data in between equals the same chain with the slices taken on the host
  { const M = 48, N = 40, k = 7, a = new Float64Array(M * N);
    for (let i = 0; i < a.length; i++) a[i] = Math.sin(1 + i * 0.37) + (i % N === Math.floor(i / N) ? 2 : 0);
    const [U, sv, V] = L.svd_decomp(L.to_device(host({shape: [M, N], dtype: 'float64', data: a})));
    const Uk = U.sliceElems('...', [0, k]), sk = sv.sliceElems([0, k]), Vk = V.sliceElems([0, k]);
    const Ak = L.matmul(Uk, L.diag_mat(sk), Vk);
    assert([U, sv, V, Uk, sk, Vk].every(x => x instanceof L.DeviceNDArray && x._host === null), 'the chain read .data');
    assert.deepStrictEqual([Array.from(Uk.shape), Array.from(sk.shape), Array.from(Vk.shape), Array.from(Ak.shape)], [[M, k], [k], [k, N], [M, N]]);
    const hU = new Float64Array(M * k), hV = V.data.slice(0, k * N), hs = sv.data.slice(0, k), R = U.shape[1];
    for (let i = 0; i < M; i++) for (let j = 0; j < k; j++) hU[i * k + j] = U.data[i * R + j];
    const up = (shape, data) => L.to_device(host({shape, dtype: 'float64', data}));
    sameWords(Ak.data, L.matmul(up([M, k], hU), L.diag_mat(up([k], hs)), up([k, N], hV)).data, 'truncated SVD');
    sameWords(Uk.data, hU, 'U[:, :k]'); sameWords(Vk.data, hV, 'V[:k, :]'); sameWords(sk.data, hs, 'sv[:k]'); }
  // reshape shares the buffer: dispose() on one releases the other
  { const dA = L.to_device(host(load(m.inputs.A_4x6))), R = dA.reshape(-1, 3);
    assert.strictEqual(R._buf, dA._buf);
    assert.deepStrictEqual(Array.from(R.shape), [8, 3]);
    sameWords(R.data, load(m.inputs.A_4x6).data, 'reshape');
    const R2 = dA.reshape(2, 12);
    dA.dispose();
    assert.throws(() => R2.data, /^Error: nd4hip: device array was disposed\.$/);
    assert.throws(() => R2.sliceElems(0), /^Error: nd4hip: device array was disposed\.$/);
    assert.throws(() => R2.reshape(24), /^Error: nd4hip: device array was disposed\.$/); }
  console.log('node slice gpu checks ok');
} else throw new Error('mode');
