'use strict';
/* Node-side checks of la.zip_elems, DeviceNDArray.mapElems and DeviceNDArray.reduceElems through the JS host and the N-API addon.
 * Driven by tests/test_node_elem.py. Comparisons are of the 32-bit words of the buffers where the expected value is not a NaN, and
 * of NaN-ness where it is: no tolerance.
 *   node node_elem_checks.js cpu <golden dir>                  (no GPU: the JS planners and the package's `math` closures evaluated on
 *                                                               the host against every fixture, every refusal of the manifest with
 *                                                               its recorded text, the refusals that come before any device work)
 *   node node_elem_checks.js install <reference dist/nd.js>    (la.zip_elems present and not enumerable after install, nd.zip_elems and
 *                                                               Object.keys(nd.la) untouched)
 *   node node_elem_checks.js gpu <golden dir> [<dist/nd.js>]   (GPU: every fixture on device arrays; device results against the host
 *                                                               module's zip_elems / mapElems / reduceElems on the same data: the real
 *                                                               bundle where the path exists, otherwise a small host module written
 *                                                               here; mixed residency; a chain that stays on the device)
 */
const fs = require('fs'), path = require('path');
const la = require(path.join(__dirname, '..', '..', 'nd4js_amd', 'js'));
const assert = require('assert');
const mode = process.argv[2];

function loadNpy(file) {
  const buf = fs.readFileSync(file), hlen = buf.readUInt16LE(8), hdr = buf.toString('latin1', 10, 10 + hlen);
  const shape = /'shape': \(([^)]*)\)/.exec(hdr)[1].split(',').filter(x => x.trim()).map(Number);
  const body = buf.slice(10 + hlen), ab = body.buffer.slice(body.byteOffset, body.byteOffset + body.byteLength);
  return {data: new Float64Array(ab), shape};
}
function sameBits(a, b, what) {
  assert(a instanceof Float64Array && b instanceof Float64Array, what);
  assert.strictEqual(a.length, b.length, what);
  const x = new Uint32Array(a.buffer, a.byteOffset, 2 * a.length), y = new Uint32Array(b.buffer, b.byteOffset, 2 * b.length);
  for (let i = 0; i < a.length; i++) {
    if (Number.isNaN(b[i])) assert(Number.isNaN(a[i]), `${what}: element ${i} is ${a[i]}, the reference has NaN`);
    else assert(x[2 * i] === y[2 * i] && x[2 * i + 1] === y[2 * i + 1], `${what}: element ${i} is ${a[i]}, the reference has ${b[i]}`);
  }
}
const prod = s => Array.from(s).reduce((x, y) => x * y, 1);
function fixtures(dir) {
  const G = path.join(dir, 'elem'), m = JSON.parse(fs.readFileSync(path.join(G, 'manifest.json')));
  return {m, load: entry => loadNpy(path.join(G, entry.file))};
}
const inputsOf = (m, load, c) => (c.arrays || [c.A]).map(n => load(m.inputs[n]));
const rowMajor = shape => { const st = new Array(shape.length); let s = 1; for (let d = shape.length - 1; d >= 0; d--) { st[d] = s; s *= shape[d]; } return st; };
const axesOf = (c, mk) => c.axes_int32 ? mk(Int32Array.of(c.axes.length), Int32Array.from(c.axes)) : c.axes;

// one recorded zip / map case from zipPlan and the closure alone, box by box as the device path goes
function plannedZip(c, ins, f) {
  const p = la.zipPlan(ins.map(a => a.shape)), out = new Float64Array(prod(p.shape)), b = p.box, cs = rowMajor(b.shape), n = prod(b.shape);
  assert(b.shape.length <= 8);
  for (const offs of b.loop) {
    const idx = new Array(b.shape.length).fill(0);
    for (let e = 0; e < n; e++) {
      const at = ins.map((_, k) => offs[k] + idx.reduce((s, i, d) => s + i * b.strides[k][d], 0));
      at.forEach((o, k) => assert(o >= 0 && o < ins[k].data.length, 'the plan leaves its operand'));
      out[offs[ins.length] + idx.reduce((s, i, d) => s + i * cs[d], 0)] = f(...at.map((o, k) => ins[k].data[o]));
      for (let d = idx.length - 1; d >= 0; d--) { if (++idx[d] < b.shape[d]) break; idx[d] = 0; }
    }
  }
  return {shape: p.shape, data: out};
}
// one recorded reduction from reducePlan and the closure alone: per launch the first element met is copied, acc = f(x, acc) after
function plannedReduce(c, A, f, axes) {
  const p = la.reducePlan(A.shape, axes), b = p.box, out = new Float64Array(prod(p.shape)), st = rowMajor(b.shape);
  const ost = new Array(b.shape.length).fill(0); let s = 1;
  for (let d = b.shape.length - 1; d >= 0; d--) if (!b.flags[d]) { ost[d] = s; s *= b.shape[d]; }
  assert(b.shape.length <= 8 && b.flags.every((fl, d) => d === 0 || fl !== b.flags[d - 1]), 'kept and reduced axes alternate');
  for (const [ao, co] of b.loop) {
    const idx = new Array(b.shape.length).fill(0), seen = new Uint8Array(s);
    for (let e = 0, n = prod(b.shape); e < n; e++) {
      const o = idx.reduce((t, i, d) => t + i * ost[d], 0), x = A.data[ao + idx.reduce((t, i, d) => t + i * st[d], 0)];
      out[co + o] = seen[o] ? f(x, out[co + o]) : x;
      seen[o] = 1;
      for (let d = idx.length - 1; d >= 0; d--) { if (++idx[d] < b.shape[d]) break; idx[d] = 0; }
    }
  }
  return {shape: p.shape, data: out};
}
function refusedCall(e) {
  if (e.fn === 'zip') return () => la.zipPlan(e.shapes);
  if (e.axes_array) {
    const a = e.axes_array, data = a.dtype === 'int32' ? Int32Array.from(a.data) : Float64Array.from(a.data);
    return () => la.reducePlan(e.a_shape, new la.NDArray(Int32Array.from(a.shape), data));
  }
  return () => la.reducePlan(e.a_shape, e.axes);
}

/* a small host module of this file's own, for the machines without the reference bundle: the semantics of nd.zip_elems,
 * NDArray.mapElems and NDArray.reduceElems on float64 arrays, written from their description */
function ownHostModule() {
  class HostNDArray {
    constructor(shape, data) { this.shape = shape; this.data = data; }
    get ndim() { return this.shape.length; }
    get dtype() { return this.data instanceof Float64Array ? 'float64' : this.data instanceof Int32Array ? 'int32' : 'object'; }
    mapElems(dtype, f) { return f == null ? new HostNDArray(this.shape, this.data.slice()) : zip_elems([this], dtype, f); }
    reduceElems(axes, dtype, f) { const r = plannedReduce(null, this, f, axes); return new HostNDArray(Int32Array.from(r.shape), r.data); }
  }
  function zip_elems(arrays, dtype, f) {
    arrays = arrays.map(a => typeof a === 'number' ? new HostNDArray(new Int32Array(0), Float64Array.of(a)) : a);
    const r = plannedZip(null, arrays, f);
    return new HostNDArray(Int32Array.from(r.shape), r.data);
  }
  const math = {add: (x, y) => x + y, sub: (x, y) => x - y, mul: (x, y) => x * y, div: (x, y) => x / y, min: (x, y) => Math.min(x, y),
                max: (x, y) => Math.max(x, y), neg: x => -x, abs: x => Math.abs(x), hypot: (x, y) => Math.hypot(x, y)};
  return {NDArray: HostNDArray, zip_elems, math, la: {matmul2: () => 'host'}, dt: {}};
}

if (mode === 'cpu') {
  const {m, load} = fixtures(process.argv[3]);
  let n = 0;
  for (const name of Object.keys(m.cases)) {
    const c = m.cases[name], want = load(c.out), ins = inputsOf(m, load, c);
    const f = c.op === null ? x => x : la.math[c.op];
    const got = c.fn === 'reduce' ? plannedReduce(c, ins[0], f, axesOf(c, (s, d) => new la.NDArray(s, d))) : plannedZip(c, ins, f);
    assert.deepStrictEqual(Array.from(got.shape), want.shape, name);
    sameBits(got.data, want.data, name);
    n++;
  }
  assert(n >= 120);
  for (const e of m.errors) assert.throws(refusedCall(e), err => err.message === e.message, `${e.fn} ${JSON.stringify(e)}: expected "${e.message}"`);
  assert(m.errors.length >= 10);
  // the planners' tables
  assert.deepStrictEqual(la.zipPlan([[70, 1], [1, 130]]).box, {shape: [70, 130], strides: [[1, 0], [0, 1]], loop: [[0, 0, 0]]});
  assert.deepStrictEqual(la.zipPlan([[], [3, 5]]).box, {shape: [15], strides: [[0], [1]], loop: [[0, 0, 0]]});
  { const p = la.zipPlan([[2, 1, 2, 1, 2, 1, 2, 1, 2, 1], [1, 2, 1, 2, 1, 2, 1, 2, 1, 2]]);
    assert.deepStrictEqual(p.box.shape, new Array(8).fill(2)); assert.strictEqual(p.box.loop.length, 4); assert.deepStrictEqual(p.box.loop[1], [0, 16, 256]); }
  assert.deepStrictEqual(la.reducePlan([2, 3, 4], [0, 2]), {shape: [3], box: {shape: [2, 3, 4], flags: [1, 0, 1], loop: [[0, 0]]}});
  assert.deepStrictEqual(la.reducePlan([2, 3, 4], -1), {shape: [2, 3], box: {shape: [6, 4], flags: [0, 1], loop: [[0, 0]]}});
  assert.deepStrictEqual(la.reducePlan(new Array(9).fill(2), [1, 3, 5, 7]).box.loop, [[0, 0], [256, 16]]);
  assert.throws(() => la.reducePlan(new Array(9).fill(2), [0, 2, 4, 6, 8]), /alternating/);
  // the methods exist; without a device array the entry refuses before anything touches a device
  for (const k of ['mapElems', 'reduceElems']) assert.strictEqual(typeof la.DeviceNDArray.prototype[k], 'function', k);
  assert.strictEqual(la.zip_elems.name, 'zip_elems');
  assert(!Object.keys(la).includes('zip_elems') && !Object.prototype.propertyIsEnumerable.call(la, 'zip_elems'), 'zip_elems must not be enumerable');
  const h = new la.NDArray(Int32Array.of(2, 2), Float64Array.of(1, 2, 3, 4));
  for (const args of [[[h, h], 'float64', 'add'], [[h, 2], 'float64', la.math.mul], [[h], 'float64', la.math.neg], [[h, h], la.math.add], [[h, h], 'int32', 'hypot']])
    assert.throws(() => la.zip_elems(...args), err => err.message === 'nd4hip.zip_elems: no device array among the arguments.');
  assert(Object.isFrozen(la.math) && ['add', 'sub', 'mul', 'div', 'min', 'max', 'neg', 'abs'].every(k => typeof la.math[k] === 'function'));
  console.log('node elem cpu checks ok');
} else if (mode === 'install') {
  const nd = require(process.argv[3]);
  const before = {zip: nd.zip_elems, laKeys: Object.keys(nd.la).join()};
  const out = la.install(nd), L = out.la;
  assert.strictEqual(typeof L.zip_elems, 'function');
  assert.strictEqual(L.zip_elems.name, 'zip_elems');
  assert(!Object.keys(L).includes('zip_elems') && !Object.prototype.propertyIsEnumerable.call(L, 'zip_elems'), 'zip_elems must not be enumerable');
  assert.strictEqual(Object.keys(nd.la).join(), before.laKeys, 'Object.keys(nd.la) changed');
  { const seen = []; for (const k in L) seen.push(k); assert(!seen.includes('zip_elems'), 'zip_elems shows up in for-in'); }
  assert.strictEqual(out.zip_elems, before.zip); assert.strictEqual(nd.zip_elems, before.zip);
  const A = nd.array('float64', [[1, 2], [3, 4]]);
  assert.throws(() => L.zip_elems([A, A], 'float64', nd.math.add), err => err.message === 'nd4hip.zip_elems: no device array among the arguments.');
  // the host module's own functions still answer host arrays
  assert.deepStrictEqual(Array.from(nd.zip_elems([A, 1], 'float64', nd.math.add).data), [2, 3, 4, 5]);
  assert.deepStrictEqual(Array.from(A.reduceElems(1, 'float64', nd.math.add).data), [3, 7]);
  console.log('node elem install checks ok');
} else if (mode === 'gpu') {
  const bundle = process.argv[4], real = !!bundle && fs.existsSync(bundle);
  const nd = real ? require(bundle) : ownHostModule();
  const L = la.install(nd).la;
  const {m, load} = fixtures(process.argv[3]);
  const host = x => new nd.NDArray(Int32Array.from(x.shape), x.data);
  const isDevice = x => x instanceof L.DeviceNDArray;
  let n = 0;
  for (const name of Object.keys(m.cases)) {
    const c = m.cases[name], want = load(c.out), ins = inputsOf(m, load, c), hs = ins.map(host), devs = hs.map(a => L.to_device(a));
    const f = c.op === null ? null : nd.math[c.op];
    let got, ref;
    if (c.fn === 'zip') { got = L.zip_elems(devs, 'float64', f); ref = nd.zip_elems(hs, 'float64', f); }
    else if (c.fn === 'map') { got = f ? devs[0].mapElems('float64', f) : devs[0].mapElems('float64'); ref = f ? hs[0].mapElems('float64', f) : hs[0].mapElems('float64'); }
    else { const ax = axesOf(c, (s, d) => new nd.NDArray(s, d)); got = devs[0].reduceElems(ax, 'float64', f); ref = hs[0].reduceElems(ax, 'float64', f); }
    assert(isDevice(got) && devs.every(d => d._host === null) && got._host === null, name + ': a device call downloaded');
    assert.strictEqual(got.dtype, 'float64', name);
    assert.deepStrictEqual(Array.from(got.shape), want.shape, name);
    sameBits(got.data, want.data, name);
    assert.deepStrictEqual(Array.from(ref.shape), want.shape, name + ' (host module)');
    sameBits(got.data, ref.data, name + ' (host module)');
    n++;
  }
  assert(n >= 120);
  // names instead of closures, the package's own closures, a copy, mixed residency and plain numbers
  { const c = m.cases.zip_div_col_row, ins = inputsOf(m, load, c), want = load(c.out);
    const col = host(ins[0]), row = host(ins[1]), dCol = L.to_device(col), dRow = L.to_device(row);
    for (const fn of ['div', la.math.div, nd.math.div]) sameBits(L.zip_elems([dCol, dRow], 'float64', fn).data, want.data, 'div by name or closure');
    sameBits(L.zip_elems([col, dRow], 'float64', 'div').data, want.data, 'host first operand');
    sameBits(L.zip_elems([dCol, row], 'float64', 'div').data, want.data, 'host second operand');
    const s = L.zip_elems([dCol, 2.5], 'float64', 'mul'), t = L.zip_elems([-0, dRow], 'float64', nd.math.max);
    assert.deepStrictEqual(Array.from(s.shape), [70, 1]); assert.deepStrictEqual(Array.from(t.shape), [1, 130]);
    sameBits(s.data, nd.zip_elems([col, 2.5], 'float64', nd.math.mul).data, 'a number as second operand');
    sameBits(t.data, nd.zip_elems([-0, row], 'float64', nd.math.max).data, 'a number as first operand');
    const copy = dCol.mapElems();
    assert(copy !== dCol && copy._buf !== dCol._buf);
    sameBits(copy.data, ins[0].data, 'mapElems()');
    const z = L.to_device(host({shape: [], data: Float64Array.of(-3)}));
    const zz = L.zip_elems([z, z], 'float64', 'mul');
    assert.deepStrictEqual(Array.from(zz.shape), []); assert.strictEqual(zz.data[0], 9);
    assert.deepStrictEqual(Array.from(dCol.reduceElems([0, 1], 'float64', 'max').shape), []); }
  // what is not accelerated is refused, and a device array is never handed to a host closure
  { const dA = L.to_device(host({shape: [4, 6], data: new Float64Array(24)})), I = L.to_device(new nd.NDArray(Int32Array.of(4, 6), new Int32Array(24)));
    let called = 0; const spy = (x, y) => { called++; return x + y; };
    const refuses = (fn, text) => assert.throws(fn, err => err.message === text, text);
    refuses(() => L.zip_elems([dA, dA], 'float64', spy), 'nd4hip.zip_elems: zip_fn is not accelerated.');
    refuses(() => L.zip_elems([dA, dA], 'float64', nd.math.hypot), 'nd4hip.zip_elems: zip_fn is not accelerated.');
    refuses(() => L.zip_elems([dA], 'float64', nd.math.min), 'nd4hip.zip_elems: zip_fn is not accelerated.');
    refuses(() => L.zip_elems([dA, dA], 'float64', nd.math.neg), 'nd4hip.zip_elems: zip_fn is not accelerated.');
    refuses(() => L.zip_elems([dA, dA], 'float64'), 'nd4hip.zip_elems: zip_fn is not accelerated.');
    refuses(() => L.zip_elems([dA, dA], nd.math.add), 'nd4hip.zip_elems: dtype is not accelerated.');
    refuses(() => L.zip_elems([dA, dA], 'object', nd.math.add), 'nd4hip.zip_elems: dtype is not accelerated.');
    refuses(() => L.zip_elems([dA, dA], 'float32', 'add'), 'nd4hip.zip_elems: dtype is not accelerated.');
    refuses(() => L.zip_elems([dA, I], 'float64', 'add'), 'nd4hip.zip_elems: dtype is not accelerated.');
    refuses(() => L.zip_elems([dA, L.to_device(host({shape: [5, 6], data: new Float64Array(30)}))], 'float64', 'add'), 'Shapes are not broadcast-compatible.');
    refuses(() => dA.mapElems(spy), 'nd4hip.mapElems: a mapper without dtype is not accelerated.');
    refuses(() => dA.mapElems('float64', spy), 'nd4hip.mapElems: mapper is not accelerated.');
    refuses(() => dA.mapElems('float64', nd.math.add), 'nd4hip.mapElems: mapper is not accelerated.');
    refuses(() => dA.mapElems('object'), 'nd4hip.mapElems: dtype is not accelerated.');
    refuses(() => I.mapElems(), 'nd4hip.mapElems: dtype is not accelerated.');
    refuses(() => dA.reduceElems(spy), 'nd4hip.reduceElems: the forms without (axes, dtype, reducer) are not accelerated.');
    refuses(() => dA.reduceElems(0, spy), 'nd4hip.reduceElems: the forms without (axes, dtype, reducer) are not accelerated.');
    refuses(() => dA.reduceElems(0, 'float64', spy), 'nd4hip.reduceElems: reducer is not accelerated.');
    refuses(() => dA.reduceElems(0, 'float64', nd.math.sub), 'nd4hip.reduceElems: reducer is not accelerated.');
    refuses(() => dA.reduceElems(0, 'float64', 'div'), 'nd4hip.reduceElems: reducer is not accelerated.');
    refuses(() => dA.reduceElems(0, 'object', nd.math.add), 'nd4hip.reduceElems: dtype is not accelerated.');
    refuses(() => I.reduceElems(0, 'float64', nd.math.add), 'nd4hip.reduceElems: dtype is not accelerated.');
    for (const e of m.errors) if (e.fn === 'reduce' && !e.axes_array) refuses(() => dA.reduceElems(e.axes, 'float64', 'add'), e.message);
    assert.strictEqual(called, 0, 'a host closure was called');
    assert(dA._host === null && I._host === null, 'a refusal downloaded'); }
  // a residual and its largest entry never leave the device: max(y - A x)
  { const M = 96, K = 80, J = 3, a = new Float64Array(M * K), x = new Float64Array(K * J), y = new Float64Array(M * J);
    for (let i = 0; i < a.length; i++) a[i] = Math.sin(1 + i * 0.37);
    for (let i = 0; i < x.length; i++) x[i] = Math.cos(2 + i * 0.11);
    for (let i = 0; i < y.length; i++) y[i] = Math.sin(3 + i * 0.05) * 7;
    const dA = L.to_device(host({shape: [M, K], data: a})), dx = L.to_device(host({shape: [K, J], data: x})), dy = L.to_device(host({shape: [M, J], data: y}));
    const Ax = L.matmul2(dA, dx), res = L.zip_elems([dy, Ax], 'float64', nd.math.sub), top = res.reduceElems([0, 1], 'float64', nd.math.max);
    assert([dA, dx, dy, Ax, res, top].every(t => isDevice(t) && t._host === null), 'the chain read .data');
    assert.deepStrictEqual(Array.from(top.shape), []);
    const hAx = host({shape: [M, J], data: Ax.data});
    const want = nd.zip_elems([host({shape: [M, J], data: y}), hAx], 'float64', nd.math.sub).reduceElems([0, 1], 'float64', nd.math.max);
    sameBits(top.data, want.data, 'max(y - A x)');
    assert(Number.isFinite(top.data[0]) && top.data[0] > 0); }
  console.log(`node elem gpu checks ok (${real ? 'reference bundle' : 'own host module'})`);
} else throw new Error('mode: cpu <golden> | install <bundle> | gpu <golden> [<bundle>]');
